"""Seeded walks over the post-mix chain and the chain's host model, with no GPU in it: tests/test_gpu_post_fuzz.py
plays a walk on a pair of twin handles, tests/test_post_walk_host.py holds the walks themselves to coverage conditions and runs them
through the model alone.

walk(seed) is a pure function of the seed and returns plain data — numbers, names and seeds, no arrays: Chain.apply makes the
coefficients, tables and responses from them with the helpers of the per-stage files, whose edge sets the draws are taken from.  Chain is
the models of those files composed in chain order; no arithmetic of its own is in it: every rule is the one a tests/test_*_host.py file
pins to numpy on bits.

Behind the limiter Chain carries the two meters of DESIGN.md 4.26 and 4.27 as test_gpu_loudness.Meter and test_gpu_spectrum.Meter
(s2r_loudness_reference and s2r_spectrum_reference with state, position and rows carried in numpy).  Their actions — METER_KINDS: set,
also while present, reset, clear, and a master fill that must be refused — come from a second generator and are spliced between the
chain's steps (_splice), which stay the ones a seed gave before the meters joined: the seeds with a history keep naming their walks.
A master fill feeds each meter that is on; Chain.meter_readings is what the getters that move nothing must then give, behind any kind
of fill, and Chain.meter_states what the getters that fetch the state's device copy give — read at a round trip, at a handover,
behind every other bus fill and panned fill (peeks) and at the end of a walk, so that master fills meet the copies both flipped
unread and fetched.

The four stages of DESIGN.md 4.28 to 4.31 are composed the same way: test_gpu_multiband.Mb between the master fader and the limiter,
test_gpu_limiter_tp.LimTp as the limiter under either detector, test_gpu_resampler.Res over the stems and the master as the caller
receives it, and test_gpu_pcm.Stage over the converter's nine outputs, or over the stems and the master without one.  Their actions —
OUTPUT_KINDS — come from a third generator (_splice_outputs) that leaves the steps of the first two what they were.  With a meter on,
neither the converter's kernel nor the PCM stage's copies the master to the pinned output, and the meters are on nearly all of a
walk: meters_pause clears the meters that are on in front of a master fill and meters_resume sets the same ones again behind it, in
front of the second generator's next action of theirs.  Chain.meter_readings carries the multiband's minima, the converter's outputs
and the PCM stage's integers and clips, Chain.meter_states the four mirrors — the limiter's among them, at its detector's sizes —,
and master_subset_walk goes through the 16 subsets of the four kernels behind the limiter on one handle."""
import numpy as np

import synth2_amd as s2
from synth2_amd import synth as s2s
from test_delay_host import FEEDS
from test_drive_host import KINDS, random_table
from test_flanger_host import INCS as FLANGER_INCS, MIXES as FLANGER_FEEDS_HOST
from test_gpu_buses import ubits
from test_gpu_chorus import INCS, SHAPES, VOICES, ChorusModel
from test_gpu_delay import DELAYS, DelayModel
from test_gpu_drive import DriveModel, oversampled
from test_gpu_dyn import COEFS, RATIOS, DynModel
from test_gpu_eq import EqModel, _coeffs
from test_gpu_flanger import SHAPE as FLANGER_SHAPE, FlangerModel
from test_gpu_limiter_tp import LimTp
from test_gpu_loudness import Meter as LoudnessMeter
from test_gpu_master import Master
from test_gpu_multiband import RATIOS as MB_RATIOS, Mb
from test_gpu_pcm import Stage, _taps
from test_gpu_resampler import Res
from test_gpu_reverb import MIXES, SR, Model, _ir
from test_gpu_room import LEVELS, RoomModel
from test_gpu_spectrum import Meter as SpectrumMeter
from test_limiter_host import PAIRS
from test_master_host import np_meters
from test_room_host import FLAT, SMALL

F = np.float32
# the default sweep of tests/test_gpu_post_fuzz.py and tests/test_post_walk_host.py: S2R_POST_FUZZ_BASE moves it, S2R_POST_FUZZ_SEEDS widens it
DEFAULT_BASE, DEFAULT_SEEDS = 5000, 32
# the seeds that found a fault, run beside the default sweep wherever it has been moved: at step 33 of 500030 and steps 19 and 63 of
# 500211 a bus fill reads PCM samples of more than max_frames frames behind the clear or the replacement of the converter that made
# them, which Synth.pcm, sizing its buffer by the converter that is set now, answered with S2R_ERR_INVALID
REGRESSION_SEEDS = (500030, 500211)
STAGES = ("eq", "dyn", "drive", "flanger", "chorus", "delay", "reverb", "room")        # chain order
INSERTS = ("eq", "dyn", "drive", "flanger", "room")
STEMS = ("chorus", "delay", "reverb")
FILLS = ("bus", "master_stems", "master", "panned")
CHAIN_KINDS = ("set", "clear", "params", "limiter_set", "limiter_clear", "limiter_ceiling", "limiter_reset", "return", "fader", "snap",
               "fill", "roundtrip", "handover")
# the meters behind the limiter and a master fill that is refused: what a second generator splices between the
# steps above (_splice), which stay what they were before the meters joined the walks
METER_KINDS = ("loudness_set", "loudness_reset", "loudness_clear", "spectrum_set", "spectrum_reset", "spectrum_clear", "refused_fill")
# the multiband compressor in front of the limiter, the limiter's detector, and the converter and the PCM stage behind the meters
# (DESIGN.md 4.28 to 4.31): what a third generator splices between the steps of the two above (_splice_outputs), which stay what they
# were.  None of them is a fill: a fill would advance the twin's voices
OUTPUT_KINDS = ("multiband_set", "multiband_params", "multiband_reset", "multiband_clear", "limiter_detector", "resampler_set", "resampler_reset",
                "resampler_clear", "pcm_set", "pcm_reset", "pcm_clear", "pcm_wrap", "meters_pause", "meters_resume")
KINDS_OF_ACTION = CHAIN_KINDS + METER_KINDS + OUTPUT_KINDS
METER_SALT = 0x6D657472                                          # the second generator's seed is seed ^ METER_SALT
OUTPUT_SALT = 0x6F757470                                         # the third generator's is seed ^ OUTPUT_SALT
# (L, M, T): the identity at (1, 1, 4); whole-table staging at L <= 64 and tile-row staging above it; ratios of a quarter and of
# 147 / 320 that make no frame of a short call; T from 4 to 64
RESAMPLER_LMT = ((1, 1, 4), (2, 1, 32), (1, 2, 64), (4, 1, 8), (1, 4, 8), (2, 3, 16), (147, 160, 48), (160, 147, 48), (147, 320, 24))
PCM_BITS, PCM_DITHERS = (8, 16, 24), ("none", "rect", "tpdf")
PCM_TAPS = (0, 1, 2, 3, 5, 7, 9)                                 # the four compiled counts (0, 1 .. 2, 3 .. 5, 6 .. 9) and those between them
PCM_T_WRAP = 2 ** 32 - 64                                        # what pcm_wrap reloads t with: the next master fill of 64 frames or more crosses 2^32
# per step and stage: an absent one is set, a present one is replaced, reset or cleared (the multiband: or given parameters); per step:
# the other detector, and with a PCM stage on a reload of t.  Chosen so that conditions 17 to 23 of tests/test_post_walk_host.py hold
P_OUT_SET, P_OUT_REPLACE, P_OUT_RESET, P_OUT_CLEAR, P_OUT_PARAMS, P_DETECTOR, P_WRAP = 0.45, 0.08, 0.04, 0.05, 0.06, 0.12, 0.05
P_PAUSE = 0.03                                                   # per step with a meter on: a master fill without the meters (meters_pause)
# hop 17 most often: the one hop here that ends on the last frame of a walker's block of eight (test_gpu_loudness.walker_distances)
LOUDNESS_HOPS, LOUDNESS_HOP_P = (16, 17, 48, 100, 4800), (0.17, 0.33, 0.2, 0.2, 0.1)
LOUDNESS_MAX_HOPS = (30, 32, 200)
# every size the spectrum kernel takes, each its own split into passes; the large ones rarely: their rows are long and their hops,
# n_fft / 8 at the least, need a walk's worth of frames
SPECTRUM_N, SPECTRUM_N_P = (256, 512, 1024, 2048, 4096, 8192), (0.24, 0.2, 0.2, 0.14, 0.14, 0.08)
SPECTRUM_WINDOWS = ("hann", "random")                            # (test_gpu_spectrum._window)
SPECTRUM_MAX_ROWS = (1, 8)
# per step and meter: an absent one is set, a present one is replaced, reset or cleared; per step: a refused fill
P_SET, P_REPLACE, P_RESET, P_CLEAR, P_REFUSED = 0.6, 0.03, 0.03, 0.02, 0.04
MAX_FRAMES = (1024, 1000, 1031, 300, 64, 2048)
# around the kernels' tiles (room 32, EQ 64, drive 240, dynamics 256, the 256-frame blocks of the meters and the limiter), the drive's
# latency of 16 and history of 32 frames, and the flanger's tile of 32 and its group of 256 frames, eight tiles whose input is loaded
# ahead: a group that ends the call and a group and one whole tile, each a frame less and a frame more too; a walk adds
# max_frames - 1 and max_frames and cuts the list to max_frames
FRAMES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 239, 240, 241, 255, 256, 257, 287, 288, 289, 300, 485, 513)
# The peak of the twin's buses: the largest magnitude of sample_buses(1024, 48000, 8) on test_gpu_reverb._handles(32) after _events
# fill 0, measured on an MI355X at commit bdd609a (the per-bus drive).  The host file scales its synthetic input to it and the
# dynamics' thresholds are set below it.
TWIN_PEAK = 2.1742098331451416
ROOMS = {"flat": FLAT, "small": SMALL}
CHORUS_H = tuple(h for h in sorted(SHAPES) if h <= 257)
DELAY_D = tuple(d for d in DELAYS if d <= 1025)
REVERB_K = (1, 40, 255, 256, 257)
# |feedback| + |cross| stays below 1, so that no line grows without bound over a walk: the host file's pairs that keep to 0.9, and two more
DELAY_FEEDS = tuple(fc for fc in FEEDS if abs(fc[0]) + abs(fc[1]) <= 0.9) + ((-0.5, 0.25), (0.3, -0.6))
DELAY_MIX = ((0.5, 1.0), (1.0, 0.5), (0.0, 1.0))
CHORUS_MIX = ((0.5, 0.25), (0.75, 0.5), (1.0, 1.0))
CHORUS_SPREAD = (0, 5, 0x40000000)
FLANGER_H = tuple(sorted(FLANGER_SHAPE))                         # every one: 33 with no depth (every tap exactly one tile old) to 4096, the ring
FLANGER_SPREAD = (0, 7, 0x40000000, 0x80000001)                  # the spreads tests/test_flanger_host.py runs its rule at
# as DELAY_FEEDS: |feedback| + |cross| stays at 0.9 or below (the per-stage file keeps its pairs at 1 over a dozen calls; a walk's line
# must not grow without bound): the host file's pairs that keep to it, (0, 0) among them, and three more, negative and both non-zero
FLANGER_FEEDS = tuple(fc for fc in FLANGER_FEEDS_HOST if abs(fc[0]) + abs(fc[1]) <= 0.9) + ((-0.5, 0.25), (0.3, -0.6), (0.0, -0.9))
FLANGER_MIX = ((0.0, 1.0), (0.5, 0.75), (1.0, 1.0), (0.25, 1.0))  # never (1, 0), an identity
DRIVE_MIX = ((0.0, 1.0), (0.5, 0.75), (0.25, 1.0))
DRIVE_PRE = (1.0, 4.0, 0.5)
DYN_BELOW_PEAK_DB = (6.0, 14.0, 24.0)                            # a threshold this far below TWIN_PEAK
LEVELS_MOVED = (1.0, 0.75, 0.5, 0.25)                            # bus returns and the master fader: never silent
BUS_WEIGHTS = np.array([5, 4, 3, 2, 1, 1, 1, 1], dtype=np.float64) / 18.0     # the low buses more often: they are in more calls


def _pick(rng, seq):
    return seq[int(rng.randint(len(seq)))]


def _shape(rng, stage):
    """what a set of `stage` is given, as names and numbers"""
    if stage == "eq":
        return dict(bands=int(rng.randint(1, 5)), seed=int(rng.randint(0, 12)))
    if stage == "dyn":
        return dict(key=int(rng.randint(0, 8)), ratio=int(rng.randint(len(RATIOS))), below=float(_pick(rng, DYN_BELOW_PEAK_DB)),
                    coefs=str(_pick(rng, sorted(COEFS))))
    if stage == "drive":
        k = int(rng.randint(len(KINDS) + 1))                     # the last one: a random table
        dry, wet = _pick(rng, DRIVE_MIX)
        return dict(curve=KINDS[k][0] if k < len(KINDS) else "random", seed=int(rng.randint(1, 20)), pre=float(_pick(rng, DRIVE_PRE)), dry=dry, wet=wet)
    if stage == "room":
        return dict(delays=str(_pick(rng, sorted(ROOMS))), levels=str(_pick(rng, sorted(LEVELS))))
    if stage == "flanger":
        fb, cross = _pick(rng, FLANGER_FEEDS)
        dry, wet = _pick(rng, FLANGER_MIX)
        return dict(H=int(_pick(rng, FLANGER_H)), inc=int(_pick(rng, FLANGER_INCS)), spread=int(_pick(rng, FLANGER_SPREAD)), feedback=float(fb), cross=float(cross),
                    dry=dry, wet=wet)
    if stage == "chorus":
        dry, wet = _pick(rng, CHORUS_MIX)
        return dict(H=int(_pick(rng, CHORUS_H)), voices=int(_pick(rng, VOICES)), inc=int(_pick(rng, INCS)), spread=int(_pick(rng, CHORUS_SPREAD)), dry=dry, wet=wet)
    if stage == "delay":
        fb, cross = _pick(rng, DELAY_FEEDS)
        dry, wet = _pick(rng, DELAY_MIX)
        return dict(D=int(_pick(rng, DELAY_D)), feedback=float(fb), cross=float(cross), dry=dry, wet=wet)
    dry, wet = _pick(rng, MIXES)
    return dict(K=int(_pick(rng, REVERB_K)), stereo=bool(rng.randint(2)), seed=int(rng.randint(1, 1000)), dry=dry, wet=wet)


def _params(rng, stage, shape):
    """(entry, the shape after it): what a kept-state entry of `stage` is given; what it cannot move — the band count, the delays, the
    history's length, the response — stays"""
    new = _shape(rng, stage)
    if stage == "eq":
        return "set_bus_eq_coeffs", dict(new, bands=shape["bands"])
    if stage == "dyn":
        return "set_bus_dynamics_params", new
    if stage == "drive":
        return "set_bus_drive_params", (new if rng.randint(2) else dict(new, curve=shape["curve"], seed=shape["seed"], table=False))
    if stage == "room":
        return "set_bus_room_params", dict(new, delays=shape["delays"])
    if stage == "flanger":                                       # (base and depth stay, and with them the line's length)
        return "set_bus_flanger_params", dict(new, H=shape["H"])
    if stage == "chorus":
        if rng.randint(2):
            return "set_bus_chorus_rate", dict(shape, inc=new["inc"], spread=new["spread"])
        return "set_bus_chorus_mix", dict(shape, dry=new["dry"], wet=new["wet"])
    if stage == "delay":
        return "set_bus_delay_mix", dict(new, D=shape["D"])
    return "set_bus_reverb_mix", dict(shape, dry=new["dry"], wet=new["wet"])


def walk(seed):
    """-> (setup, steps): setup = {"max_frames", "timing"}, steps a list of actions, each a dict with a "kind" of KINDS_OF_ACTION.  20 to
    30 steps of CHAIN_KINDS, at least 12 of them fills, and between them the meters' actions and refused fills of METER_KINDS (_splice) and the actions of OUTPUT_KINDS (_splice_outputs).  The generator keeps book of what is present, so that a clear or a kept-state entry always
    meets an effect, the limiter's ceiling always has a master fill behind it to be taken from, and a handover happens once at most.
    The last step is a master fill, so that a walk ends with every return and the master fader arrived (Master.check_committed).
    The opening takes the inserts from the seed's low five bits and the stem stages from its low three, and DEFAULT_SEEDS is 32: the
    default sweep opens on every subset of the five inserts (tests/test_post_walk_host.py asserts that all 32 are active in some fill)."""
    rng = np.random.RandomState(seed)
    max_frames = int(_pick(rng, MAX_FRAMES))
    setup = dict(max_frames=max_frames, timing=bool(rng.rand() < 0.35))
    frames = sorted({min(n, max_frames) for n in FRAMES + (max_frames - 1, max_frames)})
    n_steps = int(rng.randint(20, 31))
    fills_due = 12
    present = {st: {} for st in STAGES}                          # stage -> bus -> shape
    limiter = None
    handed = False
    steps = []
    # the opening: the subset of the inserts that the seed's last five bits name and the subset of the stem stages that its last three
    # name, on the low buses, then a bus fill and a master fill wide enough to run them — so that any 32 seeds in a row run every subset
    # of the five inserts (DEFAULT_SEEDS is 32 for that), and any 8 every subset of the stem stages in both kinds of fill
    opening = [st for j, st in enumerate(INSERTS) if seed >> j & 1] + [st for j, st in enumerate(STEMS) if seed >> j & 1]
    widest = 0
    for st in sorted(opening, key=STAGES.index):
        bus = int(rng.randint(3))
        shape = _shape(rng, st)
        if st == "dyn":
            shape["key"] = int(rng.randint(bus + 1))
        steps.append(dict(kind="set", stage=st, bus=bus, replaces=False, shape=shape))
        present[st][bus] = shape
        widest = max(widest, bus)
    for fk in (("bus", "master_stems"), ("master", "bus"))[int(rng.randint(2))]:
        n = int(_pick(rng, [q for q in frames if q >= 16]))
        steps.append(dict(kind="fill", fill=fk, n_buses=int(rng.randint(widest + 1, 9)), frames=n, tune=bool(rng.randint(2))))
        fills_due -= 1
    for k in range(len(steps), n_steps):
        left = n_steps - k
        n_present = sum(len(v) for v in present.values())
        have = [(st, bus) for st in STAGES for bus in sorted(present[st])]
        w = dict(fill=0.42, set=0.45 if n_present < 4 else 0.22 if n_present < 8 else 0.10, clear=0.10 if have else 0.0, params=0.09 if have else 0.0, master=0.12, limiter=0.10,
                 roundtrip=0.04 if have else 0.0, handover=0.05 if not handed and k >= 10 and have else 0.0)
        if left <= max(fills_due, 1):
            w = dict(fill=1.0)
        names = sorted(w)
        p = np.array([w[q] for q in names])
        kind = names[int(rng.choice(len(names), p=p / p.sum()))]
        if kind == "fill":
            fk = FILLS[int(rng.choice(4, p=[0.34, 0.28, 0.30, 0.08]))] if left > 1 else FILLS[1 + int(rng.randint(2))]
            n = int(_pick(rng, frames))
            steps.append(dict(kind="fill", fill=fk, n_buses=0 if fk == "panned" else int(rng.randint(1, 9)), frames=n, tune=bool(rng.randint(2))))
            fills_due = max(0, fills_due - 1)
        elif kind == "set":
            if have and rng.rand() < 0.3:                        # replaced while present, in mid-tail
                st, bus = have[int(rng.randint(len(have)))]
            else:
                st, bus = STAGES[int(rng.randint(len(STAGES)))], int(rng.choice(8, p=BUS_WEIGHTS))
            shape = _shape(rng, st)
            steps.append(dict(kind="set", stage=st, bus=bus, replaces=bus in present[st], shape=shape))
            present[st][bus] = shape
        elif kind == "clear":
            st, bus = have[int(rng.randint(len(have)))]
            steps.append(dict(kind="clear", stage=st, bus=bus))
            del present[st][bus]
        elif kind == "params":
            st, bus = have[int(rng.randint(len(have)))]
            entry, shape = _params(rng, st, present[st][bus])
            steps.append(dict(kind="params", stage=st, bus=bus, entry=entry, shape=shape))
            present[st][bus] = shape
        elif kind == "master":
            which = int(rng.randint(3))
            if which == 0:
                steps.append(dict(kind="return", bus=int(rng.randint(8)), level=float(_pick(rng, LEVELS_MOVED))))
            elif which == 1:
                steps.append(dict(kind="fader", level=float(_pick(rng, LEVELS_MOVED))))
            else:
                steps.append(dict(kind="snap"))
        elif kind == "limiter":
            if limiter is None:                                  # (the opening has made a master fill to take a ceiling from)
                limiter = PAIRS[int(rng.randint(len(PAIRS)))]
                steps.append(dict(kind="limiter_set", lookahead=limiter[0], hold=limiter[1]))
            else:
                which = int(rng.randint(4))
                if which == 0:
                    steps.append(dict(kind="limiter_clear"))
                    limiter = None
                elif which == 1:
                    other = [q for q in PAIRS if q != limiter]
                    limiter = other[int(rng.randint(len(other)))]
                    steps.append(dict(kind="limiter_reset", lookahead=limiter[0], hold=limiter[1]))
                else:
                    steps.append(dict(kind="limiter_ceiling", scale=float(_pick(rng, (0.5, 0.75, 1.5)))))
        elif kind == "roundtrip":
            steps.append(dict(kind="roundtrip"))
        else:
            steps.append(dict(kind="handover"))
            handed = True
    return setup, _splice_outputs(seed, setup, _splice(seed, setup, steps))


def _multiband_shape(rng, B):
    """B bands, each with a threshold below TWIN_PEAK as the bus dynamics draws it, a (ratio, knee) of test_gpu_multiband.RATIOS and
    attack and release of test_gpu_dyn.COEFS"""
    return dict(B=int(B), bands=[dict(below=float(_pick(rng, DYN_BELOW_PEAK_DB)), ratio=int(rng.randint(len(MB_RATIOS))), coefs=str(_pick(rng, sorted(COEFS))))
                                 for _ in range(B)])


def _splice_outputs(seed, setup, steps):
    """the steps with the actions of OUTPUT_KINDS between them, drawn by a third generator (seed ^ OUTPUT_SALT): the steps of
    CHAIN_KINDS and METER_KINDS stay the ones the seed gave before (tests/test_post_walk_host.py holds them to a digest).  Nothing
    goes behind the last step.  As the meters: an absent stage is set soon, a present one mostly stays.  A multiband compressor set
    while one is present takes another band count, and a resampler another (L, M, T), two times in three.  The detector is a property
    of the walk: limiter_detector re-sets a present limiter with the other one, which resets its state, and for an absent limiter
    records it for the next limiter_set — the generator reads the limiter's presence off the chain's steps."""
    rng = np.random.RandomState(seed ^ OUTPUT_SALT)
    mb = res = pcm = None
    limiter, true_peak = False, False
    loud = spec = until = None                                   # the meters' set actions, read off the steps; the step a pause of theirs ends behind
    out = []

    def other(seq, now):
        if now is not None and rng.rand() < 2.0 / 3.0:
            seq = [q for q in seq if q != now]
        return _pick(rng, seq)

    def pcm_shape():
        return dict(kind="pcm_set", replaces=pcm is not None, bits=int(_pick(rng, PCM_BITS)), dither=str(_pick(rng, PCM_DITHERS)),
                    K=int(other(PCM_TAPS, pcm and pcm["K"])), tap_seed=int(rng.randint(0, 50)), seed=int(rng.randint(0, 2 ** 31)))

    def window(k):
        """the next master fill from step k on that is not the walk's last step, if no action of the meters' lies in front of it"""
        for j in range(k, len(steps) - 1):
            if steps[j]["kind"] in METER_KINDS[:6]:
                return None
            if steps[j]["kind"] == "fill" and steps[j]["fill"] in ("master", "master_stems"):
                return j
        return None

    for k, a in enumerate(steps):
        u = rng.rand(6)
        # The meters are on nearly all of a walk, and with one on neither the converter's kernel nor the PCM stage's ever copies the
        # master out.  So now and then the meters that are on are cleared, a master fill runs without them, and the same meters are set
        # again behind it, before the second generator's next action of theirs, whose books stay right: they start afresh there.  The
        # pause runs the converter first behind the master section, or the PCM stage with no converter in front of it.
        over = window(k) if until is None and (loud or spec) and u[5] < P_PAUSE else None
        if over is not None:
            until = over
            out.append(dict(kind="meters_pause"))
            if rng.rand() < 0.5:
                if res is None:
                    res = dict(kind="resampler_set", replaces=False, **dict(zip("LMT", map(int, _pick(rng, RESAMPLER_LMT)))))
                    out.append(res)
            else:
                if res is not None:
                    out.append(dict(kind="resampler_clear"))
                    res = None
                if pcm is None:
                    pcm = pcm_shape()
                    out.append(pcm)
        if mb is None and u[0] < P_OUT_SET or mb is not None and u[0] < P_OUT_REPLACE:
            mb = dict(_multiband_shape(rng, other((1, 2, 3, 4), mb and mb["B"])), kind="multiband_set", replaces=mb is not None)
            out.append(mb)
        elif mb is not None and u[0] < P_OUT_REPLACE + P_OUT_PARAMS:
            mb = dict(_multiband_shape(rng, mb["B"]), kind="multiband_params")
            out.append(mb)
        elif mb is not None and u[0] < P_OUT_REPLACE + P_OUT_PARAMS + P_OUT_RESET:
            out.append(dict(kind="multiband_reset"))
        elif mb is not None and u[0] < P_OUT_REPLACE + P_OUT_PARAMS + P_OUT_RESET + P_OUT_CLEAR:
            out.append(dict(kind="multiband_clear"))
            mb = None
        if u[1] < P_DETECTOR:
            true_peak = not true_peak
            out.append(dict(kind="limiter_detector", true_peak=true_peak, present=limiter))
        if res is None and u[2] < P_OUT_SET or res is not None and u[2] < P_OUT_REPLACE:
            L, M, T = other(RESAMPLER_LMT, res and (res["L"], res["M"], res["T"]))
            res = dict(kind="resampler_set", replaces=res is not None, L=int(L), M=int(M), T=int(T))
            out.append(res)
        elif res is not None and u[2] < P_OUT_REPLACE + P_OUT_RESET:
            out.append(dict(kind="resampler_reset"))
        elif res is not None and u[2] < P_OUT_REPLACE + P_OUT_RESET + P_OUT_CLEAR:
            out.append(dict(kind="resampler_clear"))
            res = None
        if pcm is None and u[3] < P_OUT_SET or pcm is not None and u[3] < P_OUT_REPLACE:
            pcm = pcm_shape()
            out.append(pcm)
        elif pcm is not None and u[3] < P_OUT_REPLACE + P_OUT_RESET:
            out.append(dict(kind="pcm_reset"))
        elif pcm is not None and u[3] < P_OUT_REPLACE + P_OUT_RESET + P_OUT_CLEAR:
            out.append(dict(kind="pcm_clear"))
            pcm = None
        if pcm is not None and u[4] < P_WRAP:
            out.append(dict(kind="pcm_wrap", t=PCM_T_WRAP))
        out.append(a)
        if a["kind"] in ("limiter_set", "limiter_clear"):
            limiter = a["kind"] == "limiter_set"
        elif a["kind"] in ("loudness_set", "loudness_clear"):
            loud = a if a["kind"] == "loudness_set" else None
        elif a["kind"] in ("spectrum_set", "spectrum_clear"):
            spec = a if a["kind"] == "spectrum_set" else None
        if until == k:                                           # the meters again, in the shapes they had, behind the fill that ran without them
            out.append(dict(kind="meters_resume", loudness=loud and dict(loud, replaces=False), spectrum=spec and dict(spec, replaces=False)))
            until = None
    return out


def expanded(steps):
    """(k, action) of a walk's steps with meters_pause and meters_resume written out as the clears and sets of METER_KINDS they stand
    for, under the index of the step they came from: for the books of tests/test_post_walk_host.py"""
    loud = spec = False
    for k, a in enumerate(steps):
        if a["kind"] == "meters_pause":
            for name, there in (("loudness", loud), ("spectrum", spec)):
                if there:
                    yield k, dict(kind=name + "_clear")
        elif a["kind"] == "meters_resume":
            for name in ("loudness", "spectrum"):
                if a[name]:
                    yield k, a[name]
        else:
            yield k, a
            if a["kind"] in ("loudness_set", "loudness_clear"):
                loud = a["kind"] == "loudness_set"
            elif a["kind"] in ("spectrum_set", "spectrum_clear"):
                spec = a["kind"] == "spectrum_set"


def _spectrum_hops(n_fft):
    return (max(16, n_fft // 8), n_fft // 2, n_fft + 37)


def _splice(seed, setup, steps):
    """the steps with the actions of METER_KINDS between them, drawn by a generator of its own (seed ^ METER_SALT), so that the steps
    of CHAIN_KINDS are the ones the seed has always given, in their order (tests/test_post_walk_host.py holds them to a digest).
    Nothing goes behind the last step, which stays a master fill.  A meter that is absent is set soon and one that is present mostly
    stays: the walks are short, and a meter is worth its frames.  A spectrum meter that is set while one is present takes another
    n_fft two times in three — the state's device copies are then reserved anew at another size (S2rMirror)."""
    rng = np.random.RandomState(seed ^ METER_SALT)
    loud = spec = None
    out = []
    masters = [a["frames"] if a["kind"] == "fill" and a["fill"] in ("master", "master_stems") else 0 for a in steps]
    ahead = np.cumsum(masters[::-1])[::-1]                       # the frames of the master fills from step k on: never 0, the last step is one

    def loudness():
        return dict(kind="loudness_set", replaces=loud is not None, hop=int(LOUDNESS_HOPS[int(rng.choice(len(LOUDNESS_HOPS), p=LOUDNESS_HOP_P))]),
                    max_hops=int(_pick(rng, LOUDNESS_MAX_HOPS)))

    def spectrum(k):
        # a size whose shortest hop the master fills still to come cannot complete is not drawn: its rows would never be compared
        p = np.array(SPECTRUM_N_P) * [_spectrum_hops(n)[0] <= ahead[k] for n in SPECTRUM_N]
        if spec is not None and rng.rand() < 2.0 / 3.0:
            p[SPECTRUM_N.index(spec["n_fft"])] = 0.0
        if not p.any():
            return None
        n_fft = int(SPECTRUM_N[int(rng.choice(len(SPECTRUM_N), p=p / p.sum()))])
        return dict(kind="spectrum_set", replaces=spec is not None, n_fft=n_fft, hop=int(_pick(rng, _spectrum_hops(n_fft))),
                    window=str(_pick(rng, SPECTRUM_WINDOWS)), max_rows=int(_pick(rng, SPECTRUM_MAX_ROWS)))

    for k, a in enumerate(steps):
        u = rng.rand(3)
        if loud is None and u[0] < P_SET or loud is not None and u[0] < P_REPLACE:
            loud = loudness()
            out.append(loud)
        elif loud is not None and u[0] < P_REPLACE + P_RESET:
            out.append(dict(kind="loudness_reset"))
        elif loud is not None and u[0] < P_REPLACE + P_RESET + P_CLEAR:
            out.append(dict(kind="loudness_clear"))
            loud = None
        if spec is None and u[1] < P_SET or spec is not None and u[1] < P_REPLACE:
            new = spectrum(k)
            if new is not None:
                spec = new
                out.append(spec)
        elif spec is not None and u[1] < P_REPLACE + P_RESET:
            out.append(dict(kind="spectrum_reset"))
        elif spec is not None and u[1] < P_REPLACE + P_RESET + P_CLEAR:
            out.append(dict(kind="spectrum_clear"))
            spec = None
        if u[2] < P_REFUSED:                                     # one frame more than the handle takes: refused, and nothing moves
            out.append(dict(kind="refused_fill", n_buses=int(rng.randint(1, 9)), frames=setup["max_frames"] + 1))
        out.append(a)
    return out


class _Fan:
    """one call on every handle of a tuple, which may be empty: the host file runs the models alone"""

    def __init__(self, handles):
        self._h = tuple(handles)

    def __getattr__(self, name):
        def call(*args, **kw):
            for syn in self._h:
                getattr(syn, name)(*args, **kw)
        return call


class Chain:
    """The chain on the host: per bus EqModel, DynModel, DriveModel, FlangerModel, ChorusModel, DelayModel, the reverb's Model, RoomModel;
    behind them Master, the multiband compressor's Mb, the limiter's LimTp with either detector, the two meters, the converter's Res
    and the PCM stage's Stage.  `handles`: who else every action is performed on — (a,) on the device, () on the host."""

    def __init__(self, handles=()):
        self.handles = tuple(handles)
        self.m = dict(eq=EqModel(), dyn=DynModel(), drive=DriveModel(), flanger=FlangerModel(), chorus=ChorusModel(), delay=DelayModel(), reverb=Model(), room=RoomModel())
        self.mm, self.lim = Master(), None
        self.lims = []                                           # every LimTp the walk has had
        self.true_peak = False                                   # the detector the next limiter_set takes (limiter_detector)
        self.mb, self.res, self.pcm = None, None, None           # test_gpu_multiband.Mb, test_gpu_resampler.Res, test_gpu_pcm.Stage
        self.pcm_flat = None                                     # beside a PCM stage with taps: the same stage with none, fed the same input
        self.mbs, self.ress = [], []                             # every Mb and every Res the walk has had
        self.res_serial = 0                                      # counts the converters that started afresh: sets and resets
        # what tests/test_post_walk_host.py asks of the model alone, summed over a walk: [frames a PCM stage with taps differed from
        # its twin without, frames it converted]; [samples of the programmes that were fed that did not clip, those samples]; the
        # rails met; per resampler that ran, the programmes that sounded and those with a bit set in an output
        self.shaped, self.unclipped, self.rails, self.resampled = [0, 0], [0, 0], set(), {}
        # of the fills under the true-peak detector: [frames limited, frames whose d is not the sample magnitude on bits (LimTp.interpolated), frames]
        self.true_peak_frames = [0, 0, 0]
        self.irs = {}                                            # the responses: no entry of the library reads one back
        self.peaks = []                                          # the peak of every master of 16 frames and more so far, before the limiter
        self.lim_meters = None                                   # of the last fill that ran the limiter on the handle in hand
        self.loud, self.spec = None, None                        # the meters behind the limiter: test_gpu_loudness.Meter, test_gpu_spectrum.Meter
        self.meter_serial = 0                                    # counts the meters that started afresh: sets and resets
        # [frames in which a flanger with a feedback or a cross differed on bits from its twin without (FlangerModel), frames it ran]
        self.recursion = [0, 0]

    def of(self, stage):
        """bus -> the model's record of `stage`"""
        return getattr(self.m[stage], dict(eq="e", dyn="d", drive="d", flanger="f", chorus="c", delay="d", reverb="fx", room="r")[stage])

    def present(self):
        return " ".join("%s:%s" % (st, ",".join(str(b) for b in sorted(self.of(st)))) for st in STAGES if self.of(st)) + \
            (" multiband:%d" % self.mb.B if self.mb else "") + \
            (" limiter:%d,%d,%s" % (self.lim.L, self.lim.H, "true-peak" if self.lim.tp else "sample-peak") if self.lim else "") + \
            (" resampler:%d/%d,%d" % (self.res.L, self.res.M, self.res.T) if self.res else "") + \
            (" pcm:%d,%s,%d" % (self.pcm.bits, self.pcm.dither, self.pcm.taps.size) if self.pcm else "") + \
            (" loudness:%d,%d" % (self.loud.hop, self.loud.max_hops) if self.loud else "") + \
            (" spectrum:%d,%d,%d" % (self.spec.n, self.spec.hop, self.spec.max_rows) if self.spec else "")

    def active(self, stage, n_buses):
        """the buses on which S2rPostChain::prepare lets `stage` run in a call of n_buses"""
        if stage == "dyn":
            return [b for b in sorted(self.of(stage)) if self.m["dyn"].runs(b, n_buses)]
        return [b for b in sorted(self.of(stage)) if b < n_buses]

    # --- the actions ---
    def _args(self, stage, bus, s):
        """the arguments of `stage`'s setter and of its model's set from a shape"""
        if stage == "eq":
            c = _coeffs(s["bands"], s["seed"])
            return (c,), (c,)
        if stage == "dyn":
            ratio, knee, makeup = RATIOS[s["ratio"]]
            curve = s2.dynamics_curve(20.0 * np.log10(TWIN_PEAK) - s["below"], ratio, knee, makeup)
            return ((s["key"], curve) + COEFS[s["coefs"]](),) * 2
        if stage == "drive":
            curve = random_table(s["seed"]) if s["curve"] == "random" else s2.drive_curve(*[k for k in KINDS if k[0] == s["curve"]][0][1:])
            return ((curve, s["pre"], s["dry"], s["wet"]),) * 2
        if stage == "room":
            return ROOMS[s["delays"]] + LEVELS[s["levels"]], (ROOMS[s["delays"]], LEVELS[s["levels"]])
        if stage == "flanger":
            return (FLANGER_SHAPE[s["H"]] + (s["inc"], s["spread"], s["feedback"], s["cross"], s["dry"], s["wet"]),) * 2
        if stage == "chorus":
            return ((s["voices"],) + SHAPES[s["H"]] + (s["inc"], s["spread"], s["dry"], s["wet"]),) * 2
        if stage == "delay":
            return ((s["D"], s["feedback"], s["cross"], s["dry"], s["wet"]),) * 2
        ir = _ir(s["K"], s["seed"], s["stereo"])
        self.irs[bus] = ir
        return ((ir, s["dry"], s["wet"]),) * 2

    def apply(self, action, handles=None):
        """one action other than a fill or a handover, on the handles and on the models"""
        if handles is not None:
            self.handles = tuple(handles)
        fan, kind = _Fan(self.handles), action["kind"]
        if kind == "set":
            st, bus = action["stage"], action["bus"]
            dev, mod = self._args(st, bus, action["shape"])
            getattr(fan, "set_bus_" + dict(dyn="dynamics").get(st, st))(bus, *dev)
            self.m[st].set(bus, *mod)                            # (a set while present starts afresh, in the model too)
        elif kind == "clear":
            st, bus = action["stage"], action["bus"]
            getattr(fan, "clear_bus_" + dict(dyn="dynamics").get(st, st))(bus)
            del self.of(st)[bus]
        elif kind == "params":
            st, bus, s = action["stage"], action["bus"], action["shape"]
            f = self.of(st)[bus]
            if st == "eq":
                c = _coeffs(s["bands"], s["seed"])
                fan.set_bus_eq_coeffs(bus, c)
                f["c"] = np.array(c, dtype=F).reshape(-1, 5)
            elif st == "dyn":
                key, curve, att, rel = self._args(st, bus, s)[0]
                fan.set_bus_dynamics_params(bus, key, curve, att, rel)
                f.update(key=key, curve=np.array(curve, dtype=F), a=(F(att), F(rel)))
            elif st == "drive":
                curve, pre, dry, wet = self._args(st, bus, s)[0]
                table = s.get("table", True)
                fan.set_bus_drive_params(bus, curve if table else None, pre, dry, wet)
                f.update(pre=F(pre), dry=F(dry), wet=F(wet))
                if table:
                    f["curve"] = np.array(curve, dtype=F)
            elif st == "room":
                fan.set_bus_room_params(bus, *LEVELS[s["levels"]])
                f["lv"] = tuple(LEVELS[s["levels"]])
            elif st == "flanger":                                # (base, depth, line and phase stay)
                fan.set_bus_flanger_params(bus, s["inc"], s["spread"], s["feedback"], s["cross"], s["dry"], s["wet"])
                f.update(inc=s["inc"], spread=s["spread"], mix=(s["feedback"], s["cross"], s["dry"], s["wet"]))
            elif st == "chorus" and action["entry"] == "set_bus_chorus_rate":
                fan.set_bus_chorus_rate(bus, s["inc"], s["spread"])
                f.update(inc=s["inc"], spread=s["spread"])
            elif st == "chorus":
                fan.set_bus_chorus_mix(bus, s["dry"], s["wet"])
                f.update(dry=s["dry"], wet=s["wet"])
            elif st == "delay":
                fan.set_bus_delay_mix(bus, s["feedback"], s["cross"], s["dry"], s["wet"])
                f["mix"] = (s["feedback"], s["cross"], s["dry"], s["wet"])
            else:
                fan.set_bus_reverb_mix(bus, s["dry"], s["wet"])
                f.update(dry=s["dry"], wet=s["wet"])
        elif kind in ("limiter_set", "limiter_reset"):
            if self.lim is None:                                 # (with the walk's detector: limiter_detector)
                self.lim = LimTp(action["lookahead"], action["hold"], self.ceiling(), true_peak=self.true_peak)
                self.lims.append(self.lim)
                self.lim.set(self.handles)
            else:
                self.lim.set(self.handles, L=action["lookahead"], H=action["hold"])
        elif kind == "limiter_ceiling":
            self.lim.set(self.handles, ceiling=self.ceiling() * action["scale"])
        elif kind == "limiter_clear":
            fan.clear_master_limiter()
            self.lim = None
        elif kind == "return":
            self.mm.ret(self.handles, action["bus"], action["level"])
        elif kind == "fader":
            self.mm.fader(self.handles, action["level"])
        elif kind == "snap":
            self.mm.snap(self.handles)
        elif kind == "roundtrip":
            for syn in self.handles:
                roundtrip(self, syn)
        elif kind == "loudness_set":                             # (while one is present too: it starts afresh, in the model as on the handle)
            self.loud = LoudnessMeter(action["hop"], action["max_hops"])
            self.loud.set(*self.handles)
            self.meter_serial += 1
        elif kind == "loudness_reset":
            fan.reset_master_loudness()
            self.loud.reset()
            self.meter_serial += 1
        elif kind == "loudness_clear":
            fan.clear_master_loudness()
            self.loud = None
        elif kind == "spectrum_set":
            self.spec = SpectrumMeter(action["n_fft"], action["hop"], action["window"], action["max_rows"])
            self.spec.set(*self.handles)
            self.meter_serial += 1
        elif kind == "spectrum_reset":
            fan.reset_master_spectrum()
            self.spec.reset()
            self.meter_serial += 1
        elif kind == "spectrum_clear":
            fan.clear_master_spectrum()
            self.spec = None
        elif kind == "refused_fill":                             # the model does nothing: the call must leave everything as it was
            for syn in self.handles:
                refused_fill(syn, action)
        elif kind == "meters_pause":                             # the meters that are on, off: the next master fill runs without them
            for name, meter in (("loudness", self.loud), ("spectrum", self.spec)):
                if meter is not None:
                    self.apply(dict(kind=name + "_clear"))
        elif kind == "meters_resume":                            # ... and on again in the shapes they had: they start afresh
            for name in ("loudness", "spectrum"):
                if action[name]:
                    self.apply(action[name])
        elif kind == "limiter_detector":                         # a present limiter set again with the other detector: its state resets, in the model too
            self.true_peak = action["true_peak"]
            if self.lim is not None:
                self.lim.set(self.handles, true_peak=self.true_peak)
        elif kind in ("multiband_set", "multiband_params"):
            curves = np.stack([s2.dynamics_curve(20.0 * np.log10(TWIN_PEAK) - q["below"], *MB_RATIOS[q["ratio"]], 0.0) for q in action["bands"]])
            att, rel = [COEFS[q["coefs"]]()[0] for q in action["bands"]], [COEFS[q["coefs"]]()[1] for q in action["bands"]]
            if kind == "multiband_set":                          # (while one is present too: it starts afresh)
                self.mb = Mb(action["B"], curves, att, rel)
                self.mbs.append(self.mb)
            else:                                                # the band count and the crossover stay, and with them the state
                assert action["B"] == self.mb.B
                self.mb.curves, self.mb.att, self.mb.rel = np.array(curves, dtype=F), att, rel
            for syn in self.handles:
                self.mb.set(syn, params=kind == "multiband_params")
        elif kind == "multiband_reset":
            fan.reset_master_multiband()
            self.mb.reset()
        elif kind == "multiband_clear":
            fan.clear_master_multiband()
            self.mb = None
        elif kind == "resampler_set":
            L, M, T = action["L"], action["M"], action["T"]
            self.res = Res(L, M, np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F) if (L, M, T) == (1, 1, 4) else s2.resampler_design(L, M, T))
            self.res.set(*self.handles)
            self.ress.append(self.res)
            self.res_serial += 1
        elif kind == "resampler_reset":
            fan.reset_master_resampler()
            self.res.reset()
            self.res_serial += 1
        elif kind == "resampler_clear":
            fan.clear_master_resampler()
            self.res = None
        elif kind == "pcm_set":
            taps = _taps(action["K"], action["tap_seed"])
            self.pcm = Stage(action["bits"], action["dither"], taps, action["seed"])
            self.pcm.set(*self.handles)
            self.pcm_flat = Stage(action["bits"], action["dither"], (), action["seed"]) if action["K"] else None
        elif kind == "pcm_reset":
            fan.reset_master_pcm()
            for stage in (self.pcm, self.pcm_flat):
                if stage is not None:
                    stage.reset()
        elif kind == "pcm_clear":
            fan.clear_master_pcm()
            self.pcm = self.pcm_flat = None
        elif kind == "pcm_wrap":                                 # the present state again, with t just below 2^32: samples, counts and held clips stay
            self.pcm.load(fan, self.pcm.state.copy(), action["t"])
            if self.pcm_flat is not None:
                self.pcm_flat.t = action["t"]
        else:
            raise ValueError(kind)

    def ceiling(self):
        """half the least peak among the masters the model has computed that sounded — the limiter works on the quietest of them too —,
        and half the twin's peak while none has (behind a delay with no dry path, say)"""
        c = min(self.peaks or [TWIN_PEAK]) / 2.0
        assert 2.0 ** -20 < c < 2.0 ** 20, c
        return c

    # --- the fills ---
    def _tune(self, x, what):
        """DriveModel.tune over the drives whose bus gives it something to tune on: most of the oversampled samples are not zero, and
        their median is within reach of the largest pre"""
        view = DriveModel()
        for b, f in self.m["drive"].d.items():
            if b < x.shape[0]:
                au = np.abs(oversampled(x[b], f["hist"]))
                if (au > 0.0).mean() > 0.5 and float(np.median(au)) > 1.0 / s2.DRIVE_MAX_PRE:
                    view.d[b] = f
        view.tune(_Fan(self.handles), x, what)

    @staticmethod
    def _age(f, x):
        """the frames a room or a flanger has run behind the first frame that was not +0.0 since it was set, this call of x [N, 2]
        included (its model's record starts without one): what its lines hold is +0.0 until then"""
        age = f.get("age", 0)
        if age:
            return age + x.shape[0]
        sounding = np.nonzero(ubits(x).any(axis=1))[0]
        return x.shape[0] - int(sounding[0]) if sounding.size else 0

    def _excused(self, stage, f, x):
        """the cases a stage's own file documents as changing no bit (tests/test_gpu_chorus.py, _delay.py, _reverb.py: _fill;
        tests/test_gpu_room.py: the matrix's comment and the test with gain 0): taps that land in a history of zeros under a dry of 1, a
        response of one tap with dry 0 and wet 1 is not looked at, lines that have not turned over under a dry of 1.  The flanger has
        the chorus's case: under a dry of 1, a call whose every tap lands in a line that is +0.0 throughout — then every
        tap is +0.0, whatever feedback and cross are the line takes the bus itself, and the output is (1 * x) + (wet * +0.0), the bus.
        The chorus's bound, everything a tap of `base` frames could reach, is not enough here: a flanger's depth reaches 4063 frames
        and a phase_inc of 2^31 sends every other frame's tap to the far end of a line that is still +0.0 there while the near end
        sounds.  So the taps themselves are asked for — the rule's own (s2.flanger_reference) from the same line and phase at dry 0
        and wet 1, which returns (0 * x) + (1 * tap) — and the call is excused when none of them has a bit set.  And the room's
        case of the first turn is the flanger's too, for the room's reason, which no per-stage file meets because none puts a
        drive in front of a dry of 1: the first frames a bus sounds behind a drive are its pre-ringing, 1e-37 against a signal of
        1 (sweep seeds 200158, 200335 and 300143: a first call of 33 frames whose one tap with a bit set reads frame 0), so
        (1 * x) + (wet * tap) is x on bits by the rule.  Excused under a dry of 1 until the shortest tap, `base` frames, has
        turned over twice.  Every one of those
        files asks first that the bus is not silent as it enters: expect excuses a stage whose input is +0.0 throughout too — the first
        frames behind a delay with no dry path, say"""
        n = x.shape[0]
        if stage == "chorus":                                    # (a tap is base frames late at the least)
            line = np.concatenate([f["hist"], x], axis=0)
            return f["dry"] == 1.0 and not ubits(line[:line.shape[0] - int(np.floor(f["base"]))]).any()
        if stage == "flanger":
            if f["mix"][2] != 1.0:
                return False
            taps = s2.flanger_reference(*f["shape"], f["inc"], f["spread"], *f["mix"][:2], 0.0, 1.0, x, f["hist"], f["phase"])[0]
            return not ubits(taps).any() or self._age(f, x) <= 2 * int(np.floor(f["shape"][0]))
        if stage == "delay":
            return f["mix"][2] == 1.0 and not ubits(f["hist"][:min(n, f["D"])]).any()
        if stage == "reverb":
            return f["ir"].shape[0] == 1 and (f["dry"], f["wet"]) == (0.0, 1.0)
        if stage == "room":
            # no line is shorter than ROOM_MIN_DELAY and a set starts them as +0.0: under a dry of 1 nothing comes back before that many
            # frames have sounded, and what the first frames behind the turn bring back — a fade-in, the drive's pre-ringing — may lie
            # below half an ulp of the dry signal: excused until the shortest line has turned over twice
            return f["lv"][4] == 1.0 and self._age(f, x) <= 2 * s2.ROOM_MIN_DELAY
        return False

    def expect(self, x, action, what=""):
        """what the call of a fill action must return over the twin's dry buses x [n_buses, N, 2] (a panned fill: the twin's panned
        output, which every model leaves alone): a dict of "buses", or of "master", "stems" (where asked for), "peaks", "energies" and
        "limiter" — the limiter's meters, or the status limiter_meters() must give when no fill has run it —, with "dyn_meters", bus ->
        the least gain, of the dynamics that ran.  "trace" is for the host file: (stage, bus, changed a bit, excused) of every stage
        that ran, and "gain" the limiter's s' where it ran."""
        if action["fill"] == "panned":
            return dict(self.meter_readings(), panned=x, dyn_meters={}, trace=[])
        nb, n = x.shape[0], x.shape[1]
        assert nb == action["n_buses"] and n == action["frames"]
        y, trace = x, []
        for st in STAGES:
            act = self.active(st, nb)
            if st == "drive" and act and action["tune"]:
                self._tune(y, what)
            excused = {b: self._excused(st, self.of(st)[b], y[b]) or not ubits(y[b]).any() for b in act}     # (or the bus enters as +0.0 throughout)
            fed = {b: (self.of(st)[b]["differs"], self.of(st)[b]["frames"]) for b in act if self.of(st)[b]["mix"][:2] != (0.0, 0.0)} if st == "flanger" else {}
            z = self.m[st].expect(y)
            for b, (differs, ran) in fed.items():
                self.recursion[0] += self.of(st)[b]["differs"] - differs
                self.recursion[1] += self.of(st)[b]["frames"] - ran
            if st in ("flanger", "room"):
                for b in act:
                    self.of(st)[b]["age"] = self._age(self.of(st)[b], y[b])
            for b in range(nb):
                if b in act:
                    trace.append((st, b, not np.array_equal(ubits(z[b]), ubits(y[b])), excused[b]))
                else:
                    assert np.array_equal(ubits(z[b]), ubits(y[b])), (st, b)       # an idle stage's model passes the bus
            y = z
        out = dict(dyn_meters={b: self.of("dyn")[b]["mn"] for b in self.active("dyn", nb)}, trace=trace)
        if action["fill"] == "bus":
            out["buses"] = y
            out.update(self.meter_readings())                    # a bus fill and a panned fill move no meter
            return out
        m = self.mm.expect(y)
        # the multiband compressor between the master fader and the limiter: what it returns is the limiter's input, so the peaks'
        # bookkeeping and the ceiling read that; the master section's meters stay over m
        mi = m if self.mb is None else self.mb.expect(m)
        if n >= 16 and float(np.abs(mi).max()) > TWIN_PEAK / 64.0:
            self.peaks.append(float(np.abs(mi).max()))
        want = mi
        if self.lim is not None and 2.0 ** -19 < float(np.abs(mi).max()) <= self.lim.c:
            # the ceiling the way the per-stage walks choose it — half the peak of a master the model has computed, this one —, so that
            # every limited fill that sounds is limited: a new ceiling alone keeps the limiter's state
            self.lim.set(self.handles, ceiling=float(np.abs(mi).max()) / 2.0)
        if self.lim is not None:
            want, sp = self.lim.expect(mi)
            self.lim_meters = np.array([sp.min(), np.abs(want).max()], dtype=F)
            out["gain"] = sp
            # the true-peak detector looks at frame n - 8: a call whose magnitudes, those of the carried frames included, stay under
            # the ceiling cannot be limited, however loud its last frames are
            out["idle"] = bool(self.lim.tp and not (self.lim.d[-1] > F(self.lim.c)).any())
            if self.lim.tp:
                self.true_peak_frames[0] += int((sp < 1.0).sum())
                self.true_peak_frames[1] += int((ubits(self.lim.d[-1]) != ubits(self.lim.mag[-1])).sum())
                self.true_peak_frames[2] += n
        out["master"] = want
        out["limiter in"] = float(np.abs(mi).max())
        if action["fill"] == "master_stems":
            out["stems"] = y
        out["peaks"], out["energies"] = np_meters(y, m)          # (the master's entry is over the limiter's input)
        out["limiter"] = s2s.S2R_ERR_INVALID if self.lim_meters is None else self.lim_meters
        # the meters: the stems as the chain leaves them, n_buses of them, and the master as the caller receives it — behind the
        # limiter where one is on —, whether or not the call asks for stems (s2r.h: s2r_set_master_loudness, s2r_set_master_spectrum)
        out["meters"] = []                                       # for the host file: which programmes each meter heard, and which it read above 0.0
        for name, meter in (("loudness", self.loud), ("spectrum", self.spec)):
            if meter is not None:
                before, pos = meter.made, meter.pos
                meter.expect(y, want)
                made = meter.made - before
                new = meter.rows[len(meter.rows) - min(made, len(meter.rows)):]
                # the frames of the call that the rows it completed are taken over: up to the end of the last hop, for a spectrum the last n_fft of them
                end = made * meter.hop - pos
                heard = [q[max(0, end - meter.n) if name == "spectrum" else 0:max(0, end)] for q in list(y) + [want]]
                sounding = {p if p < nb else s2.MAX_BUSES for p, q in enumerate(heard) if q.size and float(np.abs(q).max()) > 2.0 ** -10}
                positive = {p for p in range(s2.MAX_BUSES + 1) if len(new) and (new.reshape(len(new), s2.MAX_BUSES + 1, -1)[:, p] > 0.0).any()}
                out["meters"].append(dict(name=name, instance=(self.meter_serial, id(meter)), made=made, sounding=sounding, positive=positive))
        # the converter over the same nine programmes, and the PCM stage over its outputs as eight buses and the master — over the stems
        # and the master themselves without it.  A call of which the converter makes no frame runs no PCM kernel: state, t and the
        # held clips stay, s2r_get_pcm answers 0 frames and the last call's clips are 0 (test_gpu_resampler._rfill)
        fed = list(range(nb)) + [s2.MAX_BUSES]
        stems, master = y, want
        if self.res is not None:
            ph = self.res.ph
            self.res.expect(y, want)
            stems, master = self.res.out[:s2.MAX_BUSES], self.res.out[s2.MAX_BUSES]
            book = self.resampled.setdefault(self.res_serial, [set(), set()])
            if master.shape[0]:
                # a programme has sounded where the outputs could hear it: up to the newest frame the call's last output reads (sweep
                # seed 500378: a bus behind a delay with no dry path that sounds only behind the one output of a short call)
                newest = (ph + (master.shape[0] - 1) * self.res.M) // self.res.L
                book[0] |= {p for p, q in zip(fed, list(y) + [want]) if float(np.abs(q[:newest + 1]).max()) > 2.0 ** -10}
                book[1] |= {p for p in range(s2.MAX_BUSES + 1) if ubits(self.res.out[p]).any()}
        out["count"] = master.shape[0]
        if self.pcm is not None and master.shape[0]:
            for stage in (self.pcm, self.pcm_flat):
                if stage is not None:
                    stage.expect(stems, master)
            G = 1 << (self.pcm.bits - 1)
            self.unclipped[0] += 2 * len(fed) * master.shape[0] - int(self.pcm.last.reshape(-1, 2)[fed].sum())
            self.unclipped[1] += 2 * len(fed) * master.shape[0]
            self.rails |= {name for name, rail in (("low", -G), ("high", G - 1)) if (self.pcm.pcm == rail).any()}
            if self.pcm_flat is not None:
                self.shaped[0] += int((self.pcm.pcm != self.pcm_flat.pcm).any(axis=(0, 2)).sum())
                self.shaped[1] += master.shape[0]
        elif self.pcm is not None:
            for stage in (self.pcm, self.pcm_flat):
                if stage is not None:
                    stage.pcm, stage.last = np.zeros((s2.MAX_BUSES + 1, 0, 2), dtype=np.int32), np.zeros(2 * (s2.MAX_BUSES + 1), dtype=np.uint32)
        out.update(self.meter_readings())
        return out

    def meter_readings(self):
        """what the getters that move nothing must give for the meters that are on: the stored rows and their count, and for the
        loudness meter the true peak of the last master fill and the held one"""
        out = {}
        if self.loud is not None:
            out.update({"loudness hops": len(self.loud.rows), "loudness rows": self.loud.rows.copy(), "true peak": self.loud.last.copy(),
                        "true peak held": self.loud.held.copy()})
        if self.spec is not None:
            out.update({"spectrum count": len(self.spec.rows), "spectrum rows": self.spec.rows.copy()})
        # the stages of DESIGN.md 4.28 to 4.31: the multiband's minima, the converter's outputs of all nine programmes and the PCM
        # stage's integers of the last master fill that ran each — S2R_ERR_INVALID where none has since the set or reset, or on this
        # handle —, and the clips of that fill and the held ones
        invalid = s2s.S2R_ERR_INVALID
        if self.mb is not None:
            out["multiband meters"] = invalid if self.mb.mn is None else np.array(self.mb.mn, dtype=F)
        if self.res is not None:
            out["resampled"] = invalid if self.res.out is None else self.res.out.copy()
        if self.pcm is not None:
            out.update({"pcm": invalid if self.pcm.pcm is None else self.pcm.pcm.copy(), "pcm clips": self.pcm.last.copy(), "pcm clips held": self.pcm.held.copy()})
        return out

    def meter_states(self):
        """name -> state and position of the meters that are on.  On a handle these are read through getters that fetch the state's
        device copy, which the next master fill then uploads again (S2rMirror): a walk reads them at a round trip, at a handover,
        behind every other bus fill or panned fill and at its end, and not between two master fills in a row"""
        out = {}
        for name, meter in (("loudness", self.loud), ("spectrum", self.spec)):
            if meter is not None:
                out[name + " state"], out[name + " position"] = np.array(meter.state, dtype=F), np.array([meter.pos], dtype=F)
        # the four mirrors of DESIGN.md 4.28 to 4.31, read at the same places: the multiband's state, the converter's histories and ph,
        # the PCM stage's errors and t, and the limiter's xh and gh at its detector's sizes
        if self.mb is not None:
            out["multiband state"] = np.array(self.mb.state, dtype=F)
        if self.lim is not None:
            out["limiter xh"], out["limiter gh"] = self.lim.xh, self.lim.gh
        if self.res is not None:
            out["resampler state"], out["resampler ph"] = np.array(self.res.state, dtype=F), np.array([self.res.ph], dtype=F)
        if self.pcm is not None:
            out["pcm state"], out["pcm t"] = np.array(self.pcm.state, dtype=F), _halves(self.pcm.t)
        return out

    def handed_over(self):
        """what a handover leaves on the model: the new handle's limiter has not run yet, and the held true peak is no part of a
        checkpoint (test_gpu_loudness.test_checkpoint_in_the_middle_of_a_hop), so the new handle holds +0.0 — and has made no master
        fill yet, so the true peak of its last call is +0.0 too until it makes one (seeds 5001, 5015 and 5020: a bus fill or a
        panned fill directly behind the handover)"""
        self.lim_meters = None
        if self.loud is not None:
            self.loud.held, self.loud.last = np.zeros(2, dtype=F), np.zeros(2, dtype=F)
        # s2r.h: the checkpoints of the multiband compressor, the converter and the PCM stage are the state (with ph, with t) and
        # nothing else; s2r_get_multiband_meters, s2r_get_resampled and s2r_get_pcm answer S2R_ERR_INVALID before a master fill of the
        # handle has run the stage, and the clips are counted since the set: the new handle's are 0, last and held
        if self.mb is not None:
            self.mb.mn = None
        if self.res is not None:
            self.res.out = None
        for stage in (self.pcm, self.pcm_flat):
            if stage is not None:
                stage.pcm, stage.last, stage.held = None, np.zeros_like(stage.last), np.zeros_like(stage.held)

    def states(self):
        """name -> the state every present effect and the limiter carry, as the getters of a handle give them (states_of)"""
        out = {}
        for st in STAGES:
            for b, f in self.of(st).items():
                if st in PAIRED:
                    out["%s %d history" % (st, b)], out["%s %d phase" % (st, b)] = f["hist"], _halves(f["phase"])
                else:
                    out["%s %d" % (st, b)] = np.array(f[dict(eq="st", dyn="y", drive="hist", delay="hist", reverb="hist", room="st")[st]], dtype=F)
        out.update(self.meter_states())                          # (the limiter's xh and gh among them)
        return out


def peeks(k):
    """whether the walk's step k, a bus fill or a panned fill, has the meters' state and position read behind it: every other one, so
    that a walk holds master fills directly behind a read and master fills with nothing read since the last one"""
    return k % 2 == 0


def _halves(phase):
    """a 32-bit phase as two floats that hold it exactly"""
    return np.array([int(phase) >> 16, int(phase) & 0xFFFF], dtype=F)


GETTERS = dict(eq="bus_eq_state", dyn="bus_dynamics_state", drive="bus_drive_history", flanger="bus_flanger_state", room="bus_room_state",
               chorus="bus_chorus_state", delay="bus_delay_history", reverb="bus_reverb_history")
PAIRED = ("flanger", "chorus")                                   # their state is a pair: (line, the LFO's phase)


def states_of(chain, syn):
    """Chain.states read from a handle"""
    out = {}
    for st in STAGES:
        for b in chain.of(st):
            got = getattr(syn, GETTERS[st])(b)
            if st in PAIRED:
                out["%s %d history" % (st, b)], out["%s %d phase" % (st, b)] = got[0], _halves(got[1])
            else:
                out["%s %d" % (st, b)] = np.array(got, dtype=F)
    out.update(meter_states_of(chain, syn))                      # (the limiter's xh and gh among them)
    return out


def meter_states_of(chain, syn):
    """Chain.meter_states read from a handle"""
    out = {}
    for name, meter, get in (("loudness", chain.loud, "loudness_state"), ("spectrum", chain.spec, "spectrum_state")):
        if meter is not None:
            state, pos = getattr(syn, get)()
            out[name + " state"], out[name + " position"] = np.array(state, dtype=F), np.array([pos], dtype=F)
    if chain.mb is not None:
        out["multiband state"] = syn.multiband_state()
    if chain.lim is not None:
        out["limiter xh"], out["limiter gh"] = syn.limiter_state()
    if chain.res is not None:
        state, ph = syn.resampler_state()
        out["resampler state"], out["resampler ph"] = state, np.array([ph], dtype=F)
    if chain.pcm is not None:
        state, t = syn.pcm_state()
        out["pcm state"], out["pcm t"] = state, _halves(t)
    return out


def _programmes(get):
    """all nine programmes of the last master fill through Synth.resampled or Synth.pcm, [9, frames, 2], or the status where the
    entry refuses"""
    try:
        return np.stack([get(p) for p in range(s2.MAX_BUSES + 1)])
    except s2.S2rError as err:
        return err.status


def meter_readings_of(chain, syn):
    """Chain.meter_readings read from a handle: none of these getters touches the state's copies"""
    out = {}
    if chain.loud is not None:
        out["loudness hops"], out["loudness rows"] = int(syn.get_master_loudness()[3]), syn.loudness_hops()
        out["true peak"], out["true peak held"] = syn.true_peak()
    if chain.spec is not None:
        out["spectrum count"], out["spectrum rows"] = int(syn.get_master_spectrum()[3]), syn.spectrum_rows()
    if chain.mb is not None:
        try:
            out["multiband meters"] = syn.multiband_meters()
        except s2.S2rError as err:
            out["multiband meters"] = err.status
    if chain.res is not None:
        out["resampled"] = _programmes(syn.resampled)
    if chain.pcm is not None:                                    # (the samples stay held when the converter in front is cleared or replaced: Synth.pcm)
        out["pcm"] = _programmes(syn.pcm)
        out["pcm clips"], out["pcm clips held"] = syn.pcm_clips()
    return out


def refused_fill(syn, action):
    """s2r_fill_master with one frame more than the handle takes: S2R_ERR_TOO_MANY_FRAMES, and neither buffer is written"""
    n, nb = action["frames"], action["n_buses"]
    out, st = np.full(2 * n, 7.0, dtype=F), np.full(2 * nb * n, 7.0, dtype=F)
    rc = syn.L.s2r_fill_master(syn.h, out.ctypes.data_as(s2s._f32p), st.ctypes.data_as(s2s._f32p), st.size, nb, n, SR)
    assert rc == s2s.S2R_ERR_TOO_MANY_FRAMES, "a master fill of %d frames returns %d" % (n, rc)
    assert (out == 7.0).all() and (st == 7.0).all(), "a refused master fill wrote its buffers"


def _restore(chain, syn, st, b, state):
    if st in PAIRED:
        getattr(syn, "set_" + GETTERS[st])(b, *state)
    else:
        getattr(syn, "set_" + GETTERS[st])(b, state)


def roundtrip(chain, syn):
    """every present effect's state and the limiter's out through its getter and back in through its setter"""
    for st in STAGES:
        for b in chain.of(st):
            _restore(chain, syn, st, b, getattr(syn, GETTERS[st])(b))
    if chain.lim is not None:
        syn.set_limiter_state(*syn.limiter_state())
    if chain.loud is not None:
        syn.set_loudness_state(*syn.loudness_state())
        syn.set_loudness_hops(syn.loudness_hops())
    if chain.spec is not None:
        syn.set_spectrum_state(*syn.spectrum_state())
        syn.set_spectrum_rows(syn.spectrum_rows())
    if chain.mb is not None:
        syn.set_multiband_state(syn.multiband_state())
    if chain.res is not None:
        syn.set_resampler_state(*syn.resampler_state())
    if chain.pcm is not None:                                    # (a state setter keeps the last samples and the clips: s2r.h)
        syn.set_pcm_state(*syn.pcm_state())


def copy_voices(src, dst):
    """the voices of `src`, their pans, mix and sends onto `dst`"""
    dst.import_state(src.export_state())
    dst.set_voice_pans(src.voice_pans())
    dst.set_voice_mix(*src.voice_mix())
    dst.set_voice_sends(*src.voice_sends())


def handover(chain, src, dst):
    """`dst`, a fresh handle, becomes what `src` is: the voices, every effect as src's getters give it (the reverb's response from the
    chain: no entry reads one back) with its state, the limiter with its state, the master section's applied positions and targets"""
    copy_voices(src, dst)
    for st in STAGES:
        for b in chain.of(st):
            if st == "eq":
                dst.set_bus_eq(b, src.get_bus_eq(b))
            elif st == "dyn":
                dst.set_bus_dynamics(b, *src.get_bus_dynamics(b))
            elif st == "drive":
                dst.set_bus_drive(b, *src.get_bus_drive(b))
            elif st == "flanger":
                dst.set_bus_flanger(b, *src.get_bus_flanger(b))
            elif st == "room":
                dst.set_bus_room(b, *src.get_bus_room(b))
            elif st == "chorus":
                dst.set_bus_chorus(b, *src.get_bus_chorus(b))
            elif st == "delay":
                dst.set_bus_delay(b, *src.get_bus_delay(b))
            else:
                dst.set_bus_reverb(b, chain.irs[b], *src.get_bus_reverb(b)[1:])
            _restore(chain, dst, st, b, getattr(src, GETTERS[st])(b))
    for b in range(s2.MAX_BUSES):                                # applied first, snapped, then the targets (s2r.h: s2r_snap_master)
        dst.set_bus_return(b, src.get_bus_return(b)[1])
    dst.set_master_fader(src.get_master_fader()[1])
    dst.snap_master()
    for b in range(s2.MAX_BUSES):
        dst.set_bus_return(b, src.get_bus_return(b)[0])
    dst.set_master_fader(src.get_master_fader()[0])
    mb = src.get_master_multiband()
    assert (mb is not None) == (chain.mb is not None)
    if mb is not None:                                           # every stage below: the parameters as src's getters give them, then the state
        dst.set_master_multiband(mb["curves"], mb["attack"], mb["release"], coeffs=(mb["lp"], mb["hp"], mb["ap"]) if mb["n_bands"] > 1 else None)
        dst.set_multiband_state(src.multiband_state())
    ceiling, look, hold = src.get_master_limiter()
    if look:
        dst.set_master_limiter(ceiling, look, hold, true_peak=src.get_master_limiter_detector() == s2.LIMITER_TRUE_PEAK)
        dst.set_limiter_state(*src.limiter_state())
    L, M, table = src.get_master_resampler()
    assert bool(L) == (chain.res is not None)
    if L:
        dst.set_master_resampler(L, M, table)
        dst.set_resampler_state(*src.resampler_state())
    bits, dither, taps, seed = src.get_master_pcm()
    assert bool(bits) == (chain.pcm is not None)
    if bits:
        dst.set_master_pcm(bits, dither, taps, seed)
        dst.set_pcm_state(*src.pcm_state())
    if chain.loud is not None:                                   # parameters as src's getter gives them, then state, position and rows
        c, hop, max_hops, _ = src.get_master_loudness()
        dst.set_master_loudness(SR, hop, max_hops, c)
        dst.set_loudness_state(*src.loudness_state())
        dst.set_loudness_hops(src.loudness_hops())
    if chain.spec is not None:
        n_fft, hop, max_rows, _, window = src.get_master_spectrum()
        dst.set_master_spectrum(n_fft, hop, window, max_rows)
        dst.set_spectrum_state(*src.spectrum_state())
        dst.set_spectrum_rows(src.spectrum_rows())
    chain.handed_over()
    chain.handles = (dst,)


def subset_walk():
    """the systematic complement of the seeded walks: the 32 subsets of the five inserts in Gray-code order — each step sets or clears
    exactly one insert, on two of three buses, while the others are in mid-state —, each with a bus fill, a master fill with stems and a
    master fill under the limiter, 33 frames a call, 96 calls; a chorus on bus 2 and a reverb on bus 1 stay on throughout, so the
    inserts sit in front of and behind running stem stages.  The flanger sits on bus 2 with H = 33 — every tap exactly one tile old —,
    behind a drive and in front of the chorus and a room, and on bus 1 with a feedback and a cross, in front of the reverb and a room;
    bus 0 carries none, so its launch copies that bus.  Both meters are on from the start, a loudness meter at hop 17 — the hop that
    ends on the last frame of a walker's block — and a spectrum meter at N = 1024 with a hop of 128: the 64 master fills feed them
    2112 frames through every change of inserts, with a limiter in front of them in every other one"""
    where = dict(eq=(0, 1), dyn=(1, 2), drive=(0, 2), flanger=(2, 1), room=(1, 2))
    shapes = dict(eq=[dict(bands=2, seed=1), dict(bands=4, seed=3)],
                  dyn=[dict(key=0, ratio=0, below=14.0, coefs="1ms-100ms"), dict(key=2, ratio=2, below=6.0, coefs="zero")],
                  drive=[dict(curve="hard", seed=1, pre=1.0, dry=0.0, wet=1.0), dict(curve="random", seed=5, pre=1.0, dry=0.5, wet=0.75)],
                  flanger=[dict(H=33, inc=89478 * 4, spread=0x40000000, feedback=0.7, cross=0.0, dry=0.0, wet=1.0),
                           dict(H=65, inc=89478 * 20, spread=7, feedback=-0.5, cross=0.25, dry=0.5, wet=0.75)],
                  room=[dict(delays="small", levels="dark"), dict(delays="flat", levels="hall")])
    steps = [dict(kind="set", stage="chorus", bus=2, replaces=False, shape=dict(H=145, voices=3, inc=89478 * 20, spread=0x40000000, dry=0.5, wet=0.25)),
             dict(kind="set", stage="reverb", bus=1, replaces=False, shape=dict(K=40, stereo=True, seed=77, dry=0.25, wet=1.0)),
             dict(kind="loudness_set", replaces=False, hop=17, max_hops=32),
             dict(kind="spectrum_set", replaces=False, n_fft=1024, hop=128, window="hann", max_rows=8)]
    on = 0
    for i in range(1 << len(INSERTS)):
        gray = i ^ (i >> 1)
        for j, st in enumerate(INSERTS):
            if (gray ^ on) >> j & 1:
                for bus, shape in zip(where[st], shapes[st]):
                    steps.append(dict(kind="set", stage=st, bus=bus, replaces=False, shape=shape) if gray >> j & 1 else dict(kind="clear", stage=st, bus=bus))
        on = gray
        steps.append(dict(kind="fill", fill="bus", n_buses=3, frames=33, tune=True))
        steps.append(dict(kind="fill", fill="master_stems", n_buses=3, frames=33, tune=True))
        steps.append(dict(kind="limiter_set", lookahead=5, hold=3))
        steps.append(dict(kind="fill", fill="master", n_buses=3, frames=33, tune=False))
        steps.append(dict(kind="limiter_clear"))
    return dict(max_frames=1024, timing=False), steps


MASTER_STAGES = ("loudness", "spectrum", "resampler", "pcm")     # the four kernels behind the limiter, in launch order
MASTER_SUBSET_FRAMES = (127, 128, 129, 1, 9, 257, 64, 300)       # the edges of the 128-frame tiles of the PCM and multiband kernels, which FRAMES lacks
MASTER_SUBSET_FADERS = (1.0, 0.125)                              # three buses at TWIN_PEAK: 0.125 keeps their sum inside full scale


def master_subset_walk():
    """the systematic complement of the third generator: the 16 subsets of {loudness, spectrum, resampler, PCM} in Gray-code order on
    one pair of handles — each step sets or clears exactly one of the four while the others are in mid-state —, three buses,
    max_frames 300, an EQ on bus 0 and a room on bus 1 throughout, so that the stems are not the dry buses.  Each subset gets three
    master fills: the limiter off, with the sample-peak detector, with the true-peak detector (limiter_detector on the present limiter).
    Fill f of the 48 takes MASTER_SUBSET_FRAMES[f % 8] frames, asks for stems when f / 2 is even, runs a three-band multiband
    compressor when f % 4 is 1 or 2 (set and cleared as that asks).  The master fader alternates, snapped, between 1 and 0.125 from
    subset to subset, not from fill to fill: the converter's histories carry the last 47 frames of the fill before into a fill's
    first outputs, and a subset's last fill is under the limiter, so a subset at 0.125 hears nothing louder than the ceiling from the
    subset in front of it and clips nothing on the master programme, while a subset at 1 clips there with the limiter off.  The
    resampler is (147, 160, 48), the PCM stage 16 bits with triangular dither and nine taps.  Behind every fourth subset the states
    go through a round trip, which is where a walk of master fills alone has them compared."""
    steps = [dict(kind="set", stage="eq", bus=0, replaces=False, shape=dict(bands=2, seed=1)),
             dict(kind="set", stage="room", bus=1, replaces=False, shape=dict(delays="small", levels="hall")),
             # the room rings at many times its input's level: its return brings it back to the level of a dry bus, so that the master
             # fader's low setting does what it is there for (the stems, in front of the returns, are as loud as they come)
             dict(kind="return", bus=0, level=0.5), dict(kind="return", bus=1, level=1.0 / 32.0)]
    sets = dict(loudness=dict(kind="loudness_set", replaces=False, hop=17, max_hops=32),
                spectrum=dict(kind="spectrum_set", replaces=False, n_fft=256, hop=32, window="hann", max_rows=8),
                resampler=dict(kind="resampler_set", replaces=False, L=147, M=160, T=48),
                pcm=dict(kind="pcm_set", replaces=False, bits=16, dither="tpdf", K=9, tap_seed=0, seed=77))
    band = dict(below=24.0, ratio=0, coefs="1ms-100ms")           # (24 dB below TWIN_PEAK: the bands work at the fader's low setting too)
    on, mb, f = 0, False, 0
    for i in range(1 << len(MASTER_STAGES)):
        gray = i ^ (i >> 1)
        for j, st in enumerate(MASTER_STAGES):
            if (gray ^ on) >> j & 1:
                steps.append(dict(sets[st]) if gray >> j & 1 else dict(kind=st + "_clear"))
        on = gray
        steps.append(dict(kind="fader", level=MASTER_SUBSET_FADERS[i % 2]))
        steps.append(dict(kind="snap"))
        for mode in ("off", "sample", "true"):
            if mode != "off":
                steps.append(dict(kind="limiter_detector", true_peak=mode == "true", present=mode == "true"))
            if mode == "sample":
                steps.append(dict(kind="limiter_set", lookahead=48, hold=20))
            if (f % 4 in (1, 2)) != mb:
                mb = not mb
                steps.append(dict(kind="multiband_set", replaces=False, B=3, bands=[dict(band), dict(band, ratio=1, below=14.0), dict(band, ratio=2, coefs="zero")])
                             if mb else dict(kind="multiband_clear"))
            steps.append(dict(kind="fill", fill="master_stems" if (f // 2) % 2 == 0 else "master", n_buses=3, frames=MASTER_SUBSET_FRAMES[f % 8], tune=False))
            f += 1
        steps.append(dict(kind="limiter_clear"))
        if i % 4 == 3:
            steps.append(dict(kind="roundtrip"))
    return dict(max_frames=300, timing=False), steps
