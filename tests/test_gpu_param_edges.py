"""Parity at the ends of the value ranges the C ABI accepts: every MIDI note at sample rates from 1 Hz to 0xffffffff Hz, any
pitch_hz a caller of s2r_process_layers may hand over (periods from far below one sample to far above 2^24), cutoffs from 0 to
FLT_MAX, envelope times from 0 to FLT_MAX ms with sustains down to the smallest denormal, the dsp_filters.rs / SVF coefficients at
theta far beyond pi, and each range's border seen from outside (refused, the handle unharmed).  The rest of the suite stays in the
middle of these ranges (notes 20 .. 119, 20 .. 9000 Hz, nine sample rates, envelope times of 0.25 .. 375 ms).

Every comparison goes through helpers.assert_bits_equal_finite: the oracle's samples are finite (an input for which they are not
is a badly chosen input, not a case) and the GPU's have their bit patterns — no NaN allowance, +0 and -0 differ, denormals count.
Seeds are fixed; every message names the case (parameter values as hex floats) and the first differing voice / layer and frame.
The code sites each test reaches are named in its docstring."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import Pair, assert_bits_equal_finite, make_patch, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2
from synth2_amd.synth import S2R_ERR_INVALID, S2R_ERR_PATCH_RANGE

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
DENORM_MIN = F32(2.0 ** -149)
NORMAL_MIN = F32(2.0 ** -126)
NOEV = np.zeros(0, dtype=s2.NOTE_EVENT_DTYPE)
BUF = 1031                          # 64 chunks of 16 frames and a scalar tail of 7
OSCS = [s2.OSC_SQUARE, s2.OSC_SAW, s2.OSC_TRIANGLE, s2.OSC_SINE, s2.OSC_DPW_SAW, s2.OSC_DPW_SQUARE, s2.OSC_DPW_TRIANGLE]


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _hx(x):
    return float(F32(x)).hex()


def _succ(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def _pred(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def _patch_text(p):
    return "osc %d gain %s noise %s lpf %d freq %s damping %s q %s amp %s mod %s fm %s to_lpf %s" % (
        p.osc_kind, _hx(p.osc_gain), _hx(p.noise), p.lpf_kind, _hx(p.lpf_freq), _hx(p.lpf_damping), _hx(p.lpf_q),
        "/".join(_hx(x) for x in (p.amp_env.attack_ms, p.amp_env.decay_ms, p.amp_env.sustain, p.amp_env.release_ms)),
        "/".join(_hx(x) for x in (p.mod_env.attack_ms, p.mod_env.decay_ms, p.mod_env.sustain, p.mod_env.release_ms)),
        _hx(p.mod_env_to_osc_freq), _hx(p.mod_env_to_lpf_freq))


def _copy_patch(p):
    q = s2.Patch()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(s2.Patch))
    return q


# ---- one oracle pool, several GPU handles that render the same patch and events each in its own form ----

def _form(name, out, **kw):
    """out: "rows" (s2r_render_voices) or "mix" (s2r_fill); block: block_voices; resident: s2r_set_resident; coeff: the argument of
    s2r_set_coeff_stream; flat: s2r_set_flat_shortcut; pad_bank: the patch as entry 1 of a two-patch bank (the per-lane-patch
    kernel), every voice on program 1"""
    return dict(name=name, out=out, **kw)


ROWS, MIX = _form("launch per fill", "rows"), _form("launch per fill", "mix")


class _Forms:
    def __init__(self, voices, max_frames, forms):
        f0 = forms[0]
        self.pair = Pair(voices, None, max_frames=max_frames, block_voices=f0.get("block", 0))
        self.cpu = self.pair.cpu
        self.forms = forms
        self.gpus = [self.pair.gpu] + [s2.Synth(voices, max_frames=max_frames, block_voices=f.get("block", 0)) for f in forms[1:]]
        for g, f in zip(self.gpus, forms):
            if not f.get("flat", True):
                g.set_flat_shortcut(False)
            if "coeff" in f:
                g.set_coeff_stream(f["coeff"])
            if f.get("resident"):
                g.set_resident(True)
        self.threads = _threads()
        self.note_of = {}
        self.resident_seen = {}
        self.bank_text = ""

    def set_bank(self, bank):
        """one patch, or a bank whose programs the caller then picks with program_change"""
        self.bank_text = "; ".join(_patch_text(p) for p in bank)
        if len(bank) == 1:
            self.cpu.config = oracle_cfg_from_patch(bank[0])
        else:
            self.cpu.set_bank([oracle_cfg_from_patch(p) for p in bank])
        for g, f in zip(self.gpus, self.forms):
            if len(bank) > 1:
                g.set_patch_bank(bank)
            elif f.get("pad_bank"):
                g.set_patch_bank([make_patch(osc_kind=s2.OSC_SINE, lpf_kind=s2.FILT_LP2, lpf_freq=900.0), bank[0]])
                g.program_change(1)
            else:
                g.set_patch(bank[0])

    def program_change(self, program):
        self.cpu.program_change(program)
        for g in self.gpus:
            g.program_change(program)

    def note_on(self, note):
        v = self.pair.note_on(note)
        for g in self.gpus[1:]:
            got = g.note_on(note)
            assert got == v, "voice allocation differs between handles: %d and %d" % (got, v)
        self.note_of[v] = note
        return v

    def note_off(self, note):
        self.pair.note_off(note)
        for g in self.gpus[1:]:
            g.note_off(note)

    def step(self, frames, sr, what, ev=NOEV):
        """one buffer on every handle against the oracle's; `ev`: a batch of note events (timed ones: mix forms only)"""
        if ev.size:
            for g in self.gpus:
                g.note_events(ev)
        pv = self.cpu.render_events(ev, frames, sr, threads=self.threads)
        mixes = {}
        for g, f in zip(self.gpus, self.forms):
            tag = "%s, %s, sample rate %d, %d frames [%s]" % (what, f["name"], sr, frames, self.bank_text)
            try:
                if f["out"] == "rows":
                    assert_bits_equal_finite(g.render_voices(frames, sr), pv, tag + " (per-voice rows)")
                else:
                    got = g.sample(np.empty(frames, dtype=np.float32), sr)
                    if f.get("resident"):                   # (read at once: the kernel leaves after 2 ms without a command)
                        self.resident_seen[f["name"]] = g.resident_active
                    if g.block_voices not in mixes:
                        mixes[g.block_voices] = s2o.mix_tree(pv, g.block_voices, 1)
                    assert_bits_equal_finite(got, mixes[g.block_voices], tag + " (mix)")
            except AssertionError as e:
                raise AssertionError("%s; voice -> note: %s" % (e, self.note_of)) from None
        return pv

    def close(self):
        for g in self.gpus:
            g.close()


# ---- a. every MIDI note ----

FMS = [0.0, 10.0, -10.0, 0.37]
RATES = [8000, 44100, 48000, 37123, 384000]           # 37123: not on the host's list of rates divided by in three operations
EXTREME_RATES = [1, 7, 4000000, 0xffffffff]


def _note_patch(osc, fm):
    return make_patch(osc_kind=osc, mod_env_to_osc_freq=fm, noise=0.05)


def _every_note(fr, bank, sr, what, programs=None):
    """note_on(0 .. 127) on a 128-voice pool: the pitches the handle stored, then three buffers of 1031 frames, every second note
    released after the second"""
    L = s2o.lib()
    fr.set_bank(bank)
    voice_of = []
    for n in range(128):
        if programs is not None:
            fr.program_change(programs[n])
        voice_of.append(fr.note_on(n))
    want = np.array([L.s2o_note_to_pitch(n) for n in range(128)], dtype=np.float32)
    for g, f in zip(fr.gpus, fr.forms):
        assert_bits_equal_finite(g.export_state()["pitch_hz"][voice_of], want, "%s, %s: pitch_hz of notes 0 .. 127" % (what, f["name"]))
    for k in range(3):
        fr.step(BUF, sr, "%s, buffer %d" % (what, k))
        if k == 1:
            for n in range(0, 128, 2):
                fr.note_off(n)


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("osc", OSCS)
def test_every_midi_note(osc, sr):
    """Notes 0 .. 127 (the suite renders 20 .. 119): periods from 0.6 to 47 000 samples, with the oscillator's frequency swept
    over 2^[-10, 10] by the mod envelope down to 6e-4 and up to 5e7 samples.  Per-voice rows and the mix, one-pole patch, every
    oscillator kind, FM 0, +-10 and 0.37.  Sites: build_pitch_table (s2r_host.cpp); the period and its reciprocal, `off`
    returned for fmodf(off, period) under one unsigned compare, and -2 / period as -2 * RN(1 / period) (s2r_fmod_period, osc_value,
    dpw_value, s2r_kern_common.h); the sine lookup's index that rounding takes to 1024 (gather_or_default); the division by a sample
    rate in three operations or, at 37123 Hz, a true division (fast_div_rate, s2r_host.cpp)."""
    for fm in FMS:
        fr = _Forms(128, BUF, [ROWS, MIX])
        _every_note(fr, [_note_patch(osc, fm)], sr, "every note, osc %d, FM %s" % (osc, _hx(fm)))
        fr.close()


@pytest.mark.parametrize("sr", EXTREME_RATES)
@pytest.mark.parametrize("osc", [s2.OSC_SAW, s2.OSC_SINE])
def test_every_midi_note_at_the_abi_s_rate_extremes(osc, sr):
    """The same at sample rates of 1, 7, 4 000 000 and 0xffffffff Hz (any u32 > 0 is accepted): periods from 8e-5 samples (note 127
    at 1 Hz; with FM, 8e-8) to 5e8 (note 0 at 0xffffffff Hz); envelopes of a fraction of a sample and of 8.6e8 samples (no table:
    plan_tables, s2r_host.cpp); (float)sample_rate rounding 0xffffffff up to 2^32 (make_params, s2r_host.cpp)."""
    for fm in FMS:
        fr = _Forms(128, BUF, [ROWS, MIX])
        _every_note(fr, [_note_patch(osc, fm)], sr, "every note, osc %d, FM %s" % (osc, _hx(fm)))
        fr.close()


@pytest.mark.parametrize("sr", [48000, 384000])
@pytest.mark.parametrize("osc", OSCS)
def test_every_midi_note_in_the_other_render_forms(osc, sr):
    """Every note with FM +-10 through the forms a fill can take besides a launch per fill on one workgroup: the pool-resident
    kernel and the one-launch fill on two 64-voice workgroups (pool_fill and enqueue_fused, s2r_host.cpp), filter and FM coefficients computed in-lane
    instead of read from the patch's tables (s2r_set_coeff_stream(0)), and a two-patch bank with the notes dealt to both patches
    (the per-lane-patch kernel, ensure_bank, s2r_host.cpp)."""
    for fm in (10.0, -10.0):
        what = "every note, osc %d, FM %s" % (osc, _hx(fm))
        fr = _Forms(128, BUF, [_form("pool-resident", "mix", block=64, resident=True), _form("one-launch fill", "mix", block=64),
                               _form("coefficients in-lane", "rows", coeff=0), _form("coefficients in-lane", "mix", coeff=0)])
        _every_note(fr, [_note_patch(osc, fm)], sr, what)
        fr.step(16, sr, what + ", last fill")
        assert fr.resident_seen["pool-resident"], "%s: the pool-resident kernel did not take the last fill" % what
        fr.close()
        fr = _Forms(128, BUF, [_form("two-patch bank", "rows"), _form("two-patch bank", "mix")])
        _every_note(fr, [_note_patch(osc, fm), _note_patch(OSCS[(osc + 3) % 7], -fm)], sr, what, programs=[n & 1 for n in range(128)])
        fr.close()


# ---- b. any pitch ----

LAYER_STATE = ("phase_accum", "lpf_last", "filt_x1", "filt_x2", "filt_y1", "filt_y2")


def _oracle_layers(bank, layers, frames, sr):
    """the oracle's process_layer_buf_simd (process.rs:14-49) on copies of `layers`: rows, and the states afterwards"""
    L = s2o.lib()
    n = layers.size
    rows = np.zeros((n, frames), dtype=np.float32)
    after = layers.copy()
    cfgs = [oracle_cfg_from_patch(p) for p in bank]
    col = {k: layers[k].tolist() for k in ("pitch_hz", "offset", "release_offset", "has_release", "program", "phase_accum", "lpf_last",
                                           "noise_seed", "filt_x1", "filt_x2", "filt_y1", "filt_y2", "osc_z")}
    out = {k: [0.0] * n for k in LAYER_STATE + ("osc_z",)}
    row_ptr = [s2o._fp(rows[i]) for i in range(n)]

    def run(lo, hi):
        for i in range(lo, hi):
            z = col["osc_z"][i]
            none = z != z
            st = s2o.LayerState(1, col["phase_accum"][i], col["noise_seed"][i], col["lpf_last"][i], col["filt_x1"][i], col["filt_x2"][i],
                                col["filt_y1"][i], col["filt_y2"][i], 0 if none else 1, 0.0 if none else z)
            rc = L.s2o_process_layer_buf_simd(C.byref(cfgs[col["program"][i]]), C.byref(st), col["pitch_hz"][i], sr, col["offset"][i],
                                              col["has_release"][i], col["release_offset"][i], row_ptr[i], frames)
            assert rc == 0, "the oracle refuses layer %d" % i
            out["phase_accum"][i] = st.phase_accum; out["lpf_last"][i] = st.lpf_last
            out["filt_x1"][i] = st.x1; out["filt_x2"][i] = st.x2; out["filt_y1"][i] = st.y1; out["filt_y2"][i] = st.y2
            out["osc_z"][i] = st.dpw_z if st.has_z else float("nan")

    t = _threads() if frames >= 256 else 1                      # (short rows: the calls' own cost is the interpreter's)
    cuts = [n * k // t for k in range(t + 1)]
    with ThreadPoolExecutor(t) as pool:
        for f in [pool.submit(run, cuts[k], cuts[k + 1]) for k in range(t)]:
            f.result()
    for k, v in out.items():
        after[k] = np.array(v, dtype=np.float32)
    return rows, after


def _layer_text(c):
    return "pitch_hz %s, offset %d, release %s, phase_accum %s, lpf_last %s, osc_z %s, seed %d" % (
        _hx(c["pitch_hz"]), int(c["offset"]), int(c["release_offset"]) if c["has_release"] else None, _hx(c["phase_accum"]),
        _hx(c["lpf_last"]), _hx(c["osc_z"]), int(c["noise_seed"]))


def _check_layers(handles, bank, layers, frames, sr, what, oracle=None):
    """one s2r_process_layers call per handle on copies of `layers` against the oracle; returns the layers afterwards"""
    want, after = oracle or _oracle_layers(bank, layers, frames, sr)
    for name, ws in handles:
        mine = layers.copy()
        got = ws.process_layers(mine, frames, sr)
        tag = "%s, %s, sample rate %d, %d frames [%s]" % (what, name, sr, frames, "; ".join(_patch_text(p) for p in bank))
        rows_off = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) | ~np.isfinite(want).all(axis=1))[0]
        if rows_off.size:
            tag += "; %d layers off, the first: layer %d (%s)" % (rows_off.size, rows_off[0], _layer_text(layers[rows_off[0]]))
        assert_bits_equal_finite(got, want, tag + " (rows)")
        for k in LAYER_STATE:
            off = np.nonzero(mine[k].view(np.uint32) != after[k].view(np.uint32))[0]
            assert_bits_equal_finite(mine[k], after[k], "%s: %s afterwards%s" % (
                tag, k, "; first: layer %d (%s)" % (off[0], _layer_text(layers[off[0]])) if off.size else ""))
        # osc_z: NaN says "none yet" (a marker, not arithmetic); the layers that have one compare strictly
        none = np.isnan(after["osc_z"])
        assert np.array_equal(np.isnan(mine["osc_z"]), none), tag + ": which layers have an osc_z"
        assert_bits_equal_finite(mine["osc_z"][~none], after["osc_z"][~none], tag + ": osc_z afterwards")
    return after


OFFSETS = [0, 3, 16, 4800, (1 << 24) - 2064, (1 << 24) - 1040, (1 << 24) - 48, (1 << 24) - 16, (1 << 24) - 5, 1 << 24, (1 << 24) + 16,
           (1 << 24) + 4099, (1 << 25) + 7, 0x7fffff00, 0xf0000000]


def _any_pitch(rng, sr, n):
    """every MIDI pitch; sr * 2^k for k = -24 .. 24 (periods of 2^24 .. 1 .. 2^-24 samples, so sr, sr / 2 and the periods of 2^16
    and 2^24 samples among them) with the two floats on each side of each; the rest log-uniform in 2^[-60, 60]"""
    L = s2o.lib()
    midi = np.array([L.s2o_note_to_pitch(k) for k in range(128)], dtype=np.float32)
    pow2 = (np.float64(sr) * np.exp2(np.arange(-24, 25))).astype(np.float32)
    up, down = np.float32(np.inf), np.float32(0)
    near = [pow2, np.nextafter(pow2, up), np.nextafter(np.nextafter(pow2, up), up), np.nextafter(pow2, down),
            np.nextafter(np.nextafter(pow2, down), down)]
    chosen = np.concatenate([midi] + near)
    rand = np.exp2(rng.uniform(-60.0, 60.0, n - chosen.size)).astype(np.float32)
    return np.concatenate([chosen, rand])


def _any_layers(rng, sr, n):
    a = np.zeros(n, dtype=s2.LAYER_CALL_DTYPE)
    a["pitch_hz"] = _any_pitch(rng, sr, n)
    ph = rng.rand(n).astype(np.float32) * np.float32(0.999)
    sel = rng.randint(0, 6, n)                                  # the ends of Unipolar<1> that fmodf(.., 1.0) can produce
    ph[sel == 0] = 0.0
    ph[sel == 1] = DENORM_MIN
    ph[sel == 2] = F32(1.0) - F32(2.0 ** -24)
    a["phase_accum"] = ph
    a["offset"] = rng.choice(OFFSETS, n) + np.where(rng.rand(n) < 0.5, rng.randint(0, 16, n), 0)
    rel = rng.rand(n) < 0.3
    a["has_release"] = rel
    a["release_offset"] = np.where(rel, (a["offset"] * rng.rand(n)).astype(np.uint32), 0)
    a["noise_seed"] = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    a["lpf_last"] = rng.rand(n).astype(np.float32) - np.float32(0.5)
    a["osc_z"] = np.float32(np.nan)
    return a


def _pitch_patch(osc, fm, filt, noise=0.1):
    if filt == "onepole":
        p = make_patch(osc_kind=osc, mod_env_to_osc_freq=fm, noise=noise)
    else:
        p = make_patch(osc_kind=osc, mod_env_to_osc_freq=fm, noise=noise, lpf_kind=s2.FILT_SVF_LP, lpf_q=1.7, lpf_freq=1200.0,
                       mod_env_to_lpf_freq=2.0)
    p.mod_env.sustain = 0.3                                      # the FM stays on at the large offsets too
    return p


N_LAYERS = 2048


@pytest.mark.parametrize("filt", ["onepole", "svf"])
@pytest.mark.parametrize("fm", [0.0, 10.0, -10.0])
@pytest.mark.parametrize("osc", OSCS)
def test_any_pitch(osc, fm, filt):
    """s2r_process_layers takes any pitch_hz (the suite: 20 .. 9000 Hz): 2048 layers per call with the pitches of _any_pitch,
    phase_accum at +0, 2^-149 and 1 - 2^-24 and in between, offsets on both sides of 2^24 (the fills of 39 and 1024 frames cross it)
    and near 2^31 and 2^32, three calls of 16, 39 and 1024 frames that carry the layers' states on; rows and states compared.  Sites:
    as test_every_midi_note, at periods no note reaches — below 2^-24 of a sample and above 2^24 samples, exactly 1, 2^16 and 2^24
    and the floats around them (s2r_fmod_period's window); the noise hash's change of arithmetic at offset 2^24, and — with a
    noise level of exactly 0, which the one-pole patch without FM gets a second pass for — the one-pole kernel's choice of its
    chunk for offsets below 2^24 (w_small / offs_small, s2r_render_onepole.inc:257, 584); the oscillator phase's ends."""
    sr = (8000, 48000, 384000)[(osc + int(fm != 0.0) + int(fm < 0.0) + (filt == "svf")) % 3]
    rng = np.random.RandomState(7000 + 100 * osc + int(fm) + 5 * (filt == "svf"))
    ws = s2.Synth(N_LAYERS, max_frames=1024)
    for noise in ((0.1, 0.0) if fm == 0.0 and filt == "onepole" else (0.1,)):
        bank = [_pitch_patch(osc, fm, filt, noise)]
        if noise == 0.0:                                        # attacks of 1e7 ms: both envelopes still move at every offset below 2^26,
            bank[0].amp_env.attack_ms = bank[0].mod_env.attack_ms = 1e7     # so a frame time that is no longer exact shows
        ws.set_patch(bank[0])
        layers = _any_layers(rng, sr, N_LAYERS)
        if noise == 0.0:                                        # one offset per wave of 64 layers: the choice is the wave's
            layers["offset"] = np.repeat(np.resize(OFFSETS, N_LAYERS // 64), 64)
            layers["release_offset"] = np.minimum(layers["release_offset"], layers["offset"])
        for call, frames in enumerate((16, 39, 1024)):
            layers = _check_layers([("process_layers", ws)], bank, layers, frames, sr, "any pitch, osc %d, FM %s, %s, call %d" % (
                osc, _hx(fm), filt, call))
            layers["offset"] += frames
    ws.close()


TOP_PHASE = F32(1.0) - F32(2.0 ** -24)


def _denormal_period_pitches(rng, sr, fm, n):
    """pitch_hz in sr * (2^126, 2^127): the period sr / pitch_hz is a denormal in (2^-127, 2^-126) whose reciprocal and -2 / period
    are still finite; under FM of 0.05 (2^0.05 = 1.0353) neither the period nor pitch * 2^0.05 leaves"""
    lo, hi = sr * 2.0 ** 126, min(sr * 2.0 ** 127, float(FLT_MAX))             # (at 2 and 3 Hz the binade ends at FLT_MAX)
    if fm:
        hi = min(hi, sr * 2.0 ** 127 / 1.04, float(FLT_MAX) / 1.04)
    pitch = (lo + (hi - lo) * rng.uniform(0.001, 0.999, n)).astype(np.float32)
    period = (np.float32(sr) / pitch).astype(np.float32)
    assert (period > F32(2.0 ** -127)).all() and (period < NORMAL_MIN).all()
    return pitch, period


def _denormal_period_patch(osc, fm, filt, noise=0.05):
    kw = {"onepole": {}, "svf": dict(lpf_kind=s2.FILT_SVF_LP, lpf_q=1.7, lpf_freq=1200.0, mod_env_to_lpf_freq=2.0),
          "lp1": dict(lpf_kind=s2.FILT_LP1, lpf_freq=0.1, mod_env_to_lpf_freq=1.0)}[filt]          # (a cutoff below these sample rates)
    p = make_patch(osc_kind=osc, noise=noise, mod_env_to_osc_freq=fm, **kw)
    p.mod_env.decay_ms = 30000.0; p.mod_env.sustain = 0.5
    return p


@pytest.mark.parametrize("sr", [1, 2, 3])
@pytest.mark.parametrize("filt", ["onepole", "svf", "lp1", "bank"])
@pytest.mark.parametrize("fm", [0.0, 0.05])
@pytest.mark.parametrize("osc", [s2.OSC_SQUARE, s2.OSC_SAW, s2.OSC_SINE, s2.OSC_DPW_SAW, s2.OSC_DPW_SQUARE])
def test_periods_in_the_last_binade_below_the_normal_floats(osc, fm, filt, sr):
    """A DENORMAL period (_denormal_period_pitches; the triangle's -4 / period overflows there: left out): fma(period, phase, 0)
    rounds on a grid of 2^-149, and a phase of 1 - 2^-24 — or any phase near enough to 1 — gives off == period, the one way an
    oscillator's offset leaves 0 <= off < period on legal input; fmodf(off, period) is then +0 and not `off`, a saw or square
    sample +1 and not -1.  Sites: the `slow` lanes of osc_value and dpw_value (s2r_kern_common.h:250, 302; s2r_fmod_period,
    s2r_math.h:248), and the callers of the branch-free chunk, which takes `off` for the remainder and therefore must not get
    such a wave: the one-pole kernel's fast_ok / w_flat and its FM pitch bound (s2r_render_onepole.inc:215, 249, 592) with the
    one-pole patch; the general kernel's run choice (s2r_render_general.inc:653) with an SVF and an LP1 patch (its chunk with
    FILT != 0) and with a two-patch bank whose layers are dealt to both patches (the per-lane-patch kernel).  Without FM, and with
    mod_env_to_osc_freq = 0.05 over a mod envelope of 30 s (per-frame periods from the tables' FM plane, moving by up to 3.5 %
    inside the binade); 512 layers, calls of 16 and 39 frames."""
    rng = np.random.RandomState(50 + 10 * osc + sr + (7 if fm else 0) + 1000 * ["onepole", "svf", "lp1", "bank"].index(filt))
    n = 512
    a = np.zeros(n, dtype=s2.LAYER_CALL_DTYPE)
    a["pitch_hz"], period = _denormal_period_pitches(rng, sr, fm, n)
    a["phase_accum"] = np.where(rng.rand(n) < 0.5, TOP_PHASE, (1.0 - 2.0 ** -rng.uniform(1.0, 24.0, n)).astype(np.float32))
    assert np.count_nonzero((period * a["phase_accum"]).astype(np.float32) == period) > n // 4     # off == period is reached
    # one offset per 64 layers: a wave takes the branch-free chunk only when all its lanes' envelopes allow it (no threshold inside
    # the chunk, all flat or all on the tables below 2^24), which lanes at unrelated offsets never do together
    a["offset"] = np.repeat(rng.permutation(OFFSETS)[:n // 64], 64)
    a["noise_seed"] = rng.randint(0, 1 << 31, n)
    a["lpf_last"] = rng.rand(n).astype(np.float32) - np.float32(0.5)
    a["osc_z"] = np.float32(np.nan)
    ws = s2.Synth(n, max_frames=64)
    if filt == "bank":
        other = {s2.OSC_SQUARE: s2.OSC_SAW, s2.OSC_SAW: s2.OSC_SQUARE}.get(osc, s2.OSC_SAW)
        bank = [_denormal_period_patch(osc, fm, "onepole"), _denormal_period_patch(other, fm, "svf")]
        a["program"] = rng.randint(0, 2, n)
        ws.set_patch_bank(bank)
    else:
        bank = [_denormal_period_patch(osc, fm, filt)]
        ws.set_patch(bank[0])
    for call, frames in enumerate((16, 39)):
        a = _check_layers([("process_layers", ws)], bank, a, frames, sr, "denormal period, osc %d, FM %s, %s, call %d" % (
            osc, _hx(fm), filt, call))
        a["offset"] += frames
        a["phase_accum"] = np.where(rng.rand(n) < 0.5, TOP_PHASE, a["phase_accum"])   # (the phase itself falls to 0 after one frame)
    ws.close()


@pytest.mark.parametrize("sr", [1, 3])
@pytest.mark.parametrize("osc", [s2.OSC_SQUARE, s2.OSC_SAW])
def test_denormal_periods_under_fm_with_dense_timed_events(osc, sr):
    """The one-pole kernel's dense-event loop (s2r_render_onepole.inc:410: timed events within two chunks of each other, tables,
    a noise level of exactly 0, offsets that are multiples of 16) renders with the branch-free chunk and per-frame periods from
    the tables' FM plane whatever the envelopes do; pitch_hz reaches it unchecked through s2r_import_state.  64 voices started by
    note_on, then given denormal periods, phases of 1 - 2^-24 and offsets that are multiples of 16 through export_state /
    import_state; an FM patch (0.05), noise 0; two fills of 128 frames with a note_off at every 16-frame boundary.  The oracle
    is process_layer_buf_simd per voice in 16-frame calls (the pool's voices hold notes, not pitches), mixed through the GPU's
    tree.  Fails when no caller of the chunk bounds the pitch under FM; with the bound missing in the dense loop alone it
    still passes, so it is not known to keep its waves inside that loop."""
    rng = np.random.RandomState(300 + 10 * osc + sr)
    n, frames = 64, 128
    patch = _denormal_period_patch(osc, 0.05, "onepole", noise=0.0)
    # (releases of 1e6 ms: a release that ended a fraction of a sample later would put a threshold inside every chunk, and the
    # dense loop hands a chunk with a threshold inside it to the per-frame path)
    patch.amp_env.release_ms = patch.mod_env.release_ms = 1e6
    gpu = s2.Synth(n, max_frames=frames)
    gpu.set_patch(patch)
    notes = [30 + i for i in range(n)]
    voice_of = {note: gpu.note_on(note) for note in notes}
    gpu.sample(np.empty(16, dtype=np.float32), sr)               # (the note_ons applied)
    pitch, period = _denormal_period_pitches(rng, sr, 0.05, n)
    layers = np.zeros(n, dtype=s2.LAYER_CALL_DTYPE)
    layers["osc_z"] = np.float32(np.nan)
    what = "dense timed events, osc %d, sample rate %d [%s]" % (osc, sr, _patch_text(patch))
    for fill in range(2):
        st = gpu.export_state()                                  # (a phase falls to 0 after one frame: set again before each fill)
        assert st["started"].all()
        if fill == 0:
            st["pitch_hz"] = pitch
            st["current_frame_offset"] = rng.choice([160, 1600, 4800], n)   # (multiples of 16, past attack and decay)
            st["lpf_last"] = rng.rand(n).astype(np.float32) - np.float32(0.5)
        st["phase_accum"] = np.where(rng.rand(n) < 0.7, TOP_PHASE, rng.rand(n).astype(np.float32) * np.float32(0.999))
        gpu.import_state(st)
        for k_l, k_s in (("pitch_hz", "pitch_hz"), ("offset", "current_frame_offset"), ("phase_accum", "phase_accum"),
                         ("lpf_last", "lpf_last"), ("noise_seed", "noise_seed")):
            layers[k_l] = st[k_s]
        released = [note for i, note in enumerate(notes) if i % 2 == fill]
        ev = np.array(sorted(((0, note, 16 * (j % 8), 0.0) for j, note in enumerate(released)), key=lambda r: r[2]), dtype=s2.NOTE_EVENT_DTYPE)
        gpu.note_events(ev)
        got = gpu.sample(np.empty(frames, dtype=np.float32), sr)
        rows = np.zeros((n, frames), dtype=np.float32)
        for c in range(frames // 16):
            for e in ev[ev["frame"] == 16 * c]:
                v = voice_of[int(e["note"])]
                layers["has_release"][v] = 1
                layers["release_offset"][v] = layers["offset"][v]
            if c == 0:                                           # the case is what it is for: off == period on many voices
                assert np.count_nonzero((period * layers["phase_accum"]).astype(np.float32) == period) > n // 4
            rows[:, 16 * c:16 * c + 16], layers = _oracle_layers([patch], layers, 16, sr)
            layers["offset"] += 16
        assert_bits_equal_finite(rows, rows, what + ": the oracle's rows")
        assert_bits_equal_finite(got, s2o.mix_tree(rows, gpu.block_voices, 1), "%s, fill %d (mix)" % (what, fill))
        after = gpu.export_state()
        assert_bits_equal_finite(after["phase_accum"], layers["phase_accum"], "%s, fill %d: phase_accum afterwards" % (what, fill))
        assert_bits_equal_finite(after["lpf_last"], layers["lpf_last"], "%s, fill %d: lpf_last afterwards" % (what, fill))
        assert np.array_equal(after["current_frame_offset"], layers["offset"]), what
    gpu.close()


# ---- c. cutoff ----

CUTOFFS = [F32(0.0), F32(-0.0), DENORM_MIN, F32(1e-38), _pred(2.0 ** -30), F32(2.0 ** -30), _succ(2.0 ** -30), F32(20.0),
           _pred(2.0 ** 30), F32(2.0 ** 30), _succ(2.0 ** 30), F32(1e30), FLT_MAX]


@pytest.mark.parametrize("sr", [48000, 37123])
@pytest.mark.parametrize("amount", [0.0, 10.0, -10.0])
def test_onepole_cutoff_from_zero_to_flt_max(amount, sr):
    """The one-pole filter's lpf_freq at 0, -0.0 (accepted: the check is `< 0.0f`, s2r_patch.cpp:83), the smallest denormal,
    1e-38, the three floats at 2^-30 and at 2^30 — the window inside which the host switches the three-operation quotient by the
    sample rate on (make_params, s2r_host.cpp; never at 37123 Hz) — 1e30 and FLT_MAX, with mod_env_to_lpf_freq 0 and +-10 and
    a mod envelope that decays for 20 ms and then sits flat (refresh_flat's `slope == 0.0f`).  All 128 notes, three buffers, every
    second note released; coefficients from the patch's table (s2r_set_coeff_stream 1) and computed in-lane (0), and once more as
    entry 1 of a bank.  Catches a quotient used outside its verified window, a flat envelope taken for one that moves, and a table
    and an in-lane path that disagree where 2^(amount * env) * lpf_freq under- or overflows."""
    fr = _Forms(128, BUF, [_form("coefficient table", "rows", coeff=1), _form("coefficient table", "mix", coeff=1),
                           _form("coefficients in-lane", "rows", coeff=0), _form("entry 1 of a bank", "rows", pad_bank=True)])
    for f in CUTOFFS:
        p = make_patch(lpf_freq=f, mod_env_to_lpf_freq=amount, noise=0.05)
        p.mod_env.attack_ms = 0.0; p.mod_env.decay_ms = 20.0; p.mod_env.sustain = 0.25; p.mod_env.release_ms = 10.0
        _every_note(fr, [p], sr, "cutoff %s, amount %s" % (_hx(f), _hx(amount)))
    fr.close()


# ---- d. envelope times and sustain ----

SUSTAINS = [F32(0.0), DENORM_MIN, F32(1e-39), F32(1.0) - F32(2.0 ** -24), F32(1.0)]
ENV_NOTES = list(range(36, 100, 2))


def _ms_as_samples(ms, sr):
    return F32(s2o.lib().s2o_ms_as_samples(float(ms), sr))


def _env_times(sr):
    """0, the smallest denormal, 1e-6, 0.02, 1/48 ms (one sample at 48 kHz), 1e7, 1e9 (more than 2^32 samples), 1e30 and FLT_MAX
    ms; and the times for which Ms::as_samples (units.rs:44-53) lands next to 1 and next to 16 samples at this rate"""
    times = [F32(0.0), DENORM_MIN, F32(1e-6), F32(0.02), F32(1.0) / F32(48.0), F32(1e7), F32(1e9), F32(1e30), FLT_MAX]
    for k in (1, 16):
        ms = F32(k * 1000.0 / sr)
        times += [_pred(ms), ms, _succ(ms)]
        assert abs(float(_ms_as_samples(ms, sr)) - k) < 1e-3
    return times


def _env_cases(sr):
    """every time on all six places at once, then 25 seeded draws of six times"""
    times = _env_times(sr)
    rng = np.random.RandomState(4242)
    return [(t,) * 6 for t in times] + [tuple(times[i] for i in rng.randint(0, len(times), 6)) for _ in range(25)]


def _env_patch(times, sustain, k):
    p = make_patch(osc_kind=(s2.OSC_SAW, s2.OSC_SINE)[k % 2], lpf_freq=5000.0, mod_env_to_lpf_freq=2.0, mod_env_to_osc_freq=0.37,
                   noise=0.05)
    p.amp_env.attack_ms, p.amp_env.decay_ms, p.amp_env.release_ms, p.mod_env.attack_ms, p.mod_env.decay_ms, p.mod_env.release_ms = (
        float(t) for t in times)
    p.amp_env.sustain = p.mod_env.sustain = float(sustain)
    return p


def _env_events(timed):
    """buffer 0: the note_ons (timed: at frames 0, 16, .. 64); buffer 1: every second note released (timed: at 16-frame boundaries
    across the buffer; untimed: before it starts); buffer 2: none"""
    on = [(1, n, 16 * (i % 5) if timed else 0, 1.0) for i, n in enumerate(ENV_NOTES)]
    off = [(0, n, 16 * ((i * 7) % 64) if timed else 0, 0.0) for i, n in enumerate(ENV_NOTES[::2])]
    return [np.array(sorted(rows, key=lambda r: r[2]), dtype=s2.NOTE_EVENT_DTYPE) for rows in (on, off)] + [NOEV]


@pytest.mark.parametrize("sr", [48000, 8000])
@pytest.mark.parametrize("timed", [False, True])
def test_envelope_times_and_sustain_at_their_ends(timed, sr):
    """Attack, decay and release of both envelopes from 0 to FLT_MAX ms (the suite: 0 or 0.25 .. 375 ms) and sustains of 0, 2^-149,
    1e-39, 1 - 2^-24 and 1, both modulation amounts non-zero, 32 notes of which every second is released in the second buffer —
    by untimed events (per-voice rows and the mix) or by timed ones at 16-frame boundaries (the mix) — with the flat-envelope
    shortcut on and off.  Sites: resolve_env (s2r_host.cpp: 1 / A, (S - 1) / D, -S / R with A, D, R of 0, of a fraction of
    a sample, of 1 and 16 samples exactly, of more than 2^32 samples and of inf); refresh_flat's `slope == 0.0f` with a value of S or
    +0; plan_tables' cut (s2r_host.cpp).  Catches a slope or a product flushed to zero, an envelope taken for flat one chunk
    early or late, a one-sample attack off by one frame, and a frame count beyond 2^32 wrapped.

    A denormal sustain makes denormal slopes and denormal output.  Where the amp envelope reaches it within 16 samples (attack +
    decay, by Ms::as_samples), a note that is never released sits on the sustain for all but its first frames, and a product with
    2^-149 is zero only where the other factor is at most 1/2; so the test asserts that more than half of the ORACLE's samples of
    such a case's held notes are non-zero denormals (72 .. 100 % when this was written): the case then tests that nothing on the
    device path flushes to zero."""
    if timed:
        forms = [_form("timed events", "mix"), _form("timed events, no flat shortcut", "mix", flat=False)]
    else:
        forms = [ROWS, MIX, _form("no flat shortcut", "rows", flat=False)]
    fr = _Forms(len(ENV_NOTES), BUF, forms)
    events = _env_events(timed)
    for k, times in enumerate(_env_cases(sr)):
        for sustain in SUSTAINS:
            p = _env_patch(times, sustain, k)
            what = "envelope case %d, sustain %s" % (k, _hx(sustain))
            fr.set_bank([p])
            pvs = [fr.step(BUF, sr, "%s, buffer %d" % (what, b), events[b]) for b in range(3)]
            if 0.0 < sustain < NORMAL_MIN and float(_ms_as_samples(times[0], sr)) + float(_ms_as_samples(times[1], sr)) < 16.0:
                held = [i for i in range(len(ENV_NOTES)) if not fr.cpu.voice(i).has_release]
                assert len(held) == len(ENV_NOTES) // 2, (what, held)
                pv = np.concatenate(pvs, axis=1)[held]
                share = np.count_nonzero((pv != 0) & (np.abs(pv) < NORMAL_MIN)) / pv.size
                assert share > 0.5, "%s: only %.1f %% of the oracle's samples are non-zero denormals [%s]" % (what, 100 * share, _patch_text(p))
    fr.close()


# ---- e. filter coefficients without blow-up ----

FILTER_KINDS = [s2.FILT_LP1, s2.FILT_HP1, s2.FILT_LP2, s2.FILT_HP2, s2.FILT_BP2, s2.FILT_SVF_LP, s2.FILT_SVF_BP, s2.FILT_SVF_HP]
SHAPES = [F32(1e-3), F32(0.2), F32(np.sqrt(2.0)), F32(10.0)]
SWEEPS = [(F32(20000.0), 10.0), (F32(2.0 ** -20), -10.0)]     # lpf_freq * 2^[0, 10] and lpf_freq * 2^[-10, 0]
N_SWEEP = 1024


def _sweep_patch(osc, kind, lpf_freq, amount, shape):
    """damping (LP2, HP2) or q (BP2, SVF) = shape; the other one stays at its default"""
    p = make_patch(osc_kind=osc, lpf_kind=kind, lpf_freq=lpf_freq, mod_env_to_lpf_freq=amount)
    if kind >= s2.FILT_BP2:
        p.lpf_q = shape
    else:
        p.lpf_damping = shape
    p.mod_env.attack_ms = 50.0; p.mod_env.decay_ms = 50.0; p.mod_env.sustain = 0.0; p.mod_env.release_ms = 10.0
    return p


def _sweep_layers(rng, sr):
    """layers with a zero filter state at 1024 offsets along the mod envelope's attack and decay (100 ms) and a little past them
    (at 8 kHz those are 840 frames: every frame of the envelope is an offset, 183 of them twice at another pitch and phase)"""
    a = np.zeros(N_SWEEP, dtype=s2.LAYER_CALL_DTYPE)
    a["pitch_hz"] = np.exp(rng.uniform(np.log(30.0), np.log(5000.0), N_SWEEP)).astype(np.float32)
    a["offset"] = np.linspace(0.0, 0.105 * sr, N_SWEEP).astype(np.uint32)
    a["phase_accum"] = rng.rand(N_SWEEP).astype(np.float32) * np.float32(0.999)
    a["osc_z"] = np.float32(np.nan)
    return a


def _sweep(handles, kind, sr, shapes, what):
    rng = np.random.RandomState(900 + 10 * kind + sr % 7)
    for osc in (s2.OSC_SAW, s2.OSC_DPW_SAW):
        for lpf_freq, amount in SWEEPS:
            for shape in shapes:
                p = _sweep_patch(osc, kind, lpf_freq, amount, shape)
                use = handles if osc == s2.OSC_SAW else handles[:1]       # (a DPW oscillator has no coefficient table)
                for _, ws in use:
                    ws.set_patch(p)
                layers = _sweep_layers(rng, sr)
                for attempt in range(4):
                    oracle = _oracle_layers([p], layers, 16, sr)
                    unfit = ~np.isfinite(oracle[0]).all(axis=1)
                    if not unfit.any():
                        break
                    # a cutoff next to a pole of tan() can take a filter from zero to inf within 16 frames: such a layer is a badly
                    # chosen input and moves on by 37 frames — a handful at most, or the sweep itself is badly chosen
                    assert unfit.sum() <= 4, "%s: the oracle is not finite for %d of %d layers" % (what, unfit.sum(), N_SWEEP)
                    layers["offset"][unfit] += 37
                _check_layers(use, [p], layers, 16, sr, "%s, osc %d, shape %s" % (what, osc, _hx(shape)), oracle)


@pytest.mark.parametrize("sr", [8000, 48000, 384000])
@pytest.mark.parametrize("kind", FILTER_KINDS)
def test_filter_coefficients_along_a_cutoff_sweep(kind, sr):
    """The dsp_filters.rs kinds and the SVF outputs with the cutoff swept over 20000 * 2^[0, 10] Hz — theta = 2 pi f / sr up to
    16 000 rad, the large-argument paths of s2r_sinf / s2r_cosf / s2r_tanf (s2r_math.h:396-460) as the kernels call them — and
    over 2^-20 * 2^[-10, 0] Hz (theta down to 1e-13), damping / q of 1e-3, 0.2, sqrt 2 and 10 (and damping 0 where the kind reads
    damping), saw and DPW-saw input.  Each layer starts from a ZERO filter state and runs 16 frames: long enough for every
    coefficient to reach the output, too short for a filter driven unstable to overflow — the oracle stays finite, so every sample
    is compared (a NaN compares equal to a NaN in assert_bits_equal; over longer runs most of what such patches render is NaN).
    Coefficients from the table and computed in-lane.  Catches a range reduction, a coefficient formula or a table entry that is
    off at an argument the rest of the suite only reaches with NaN in the state."""
    ws = s2.Synth(N_SWEEP, max_frames=16)
    wi = s2.Synth(N_SWEEP, max_frames=16)
    wi.set_coeff_stream(0)
    shapes = SHAPES + ([F32(0.0)] if kind < s2.FILT_BP2 else [])
    _sweep([("coefficient table", ws), ("coefficients in-lane", wi)], kind, sr, shapes, "cutoff sweep, filter %d" % kind)
    ws.close()
    wi.close()


Q_FLOOR = F32(2.0 ** -100)


@pytest.mark.parametrize("kind", [s2.FILT_SVF_LP, s2.FILT_SVF_BP, s2.FILT_SVF_HP])
def test_svf_at_the_smallest_q_and_below_it(kind):
    """lpf_q = 2^-100 is the smallest the fill accepts for the SVF (check_fill, s2r_host.cpp: k = 1 / q stays finite): rendered
    over both sweeps.  The float below it passes s2r_set_patch (Unipolar<10>) and is refused by every fill with
    S2R_ERR_PATCH_RANGE; once a valid patch is set again the handle renders on from where it was, bit for bit."""
    ws = s2.Synth(N_SWEEP, max_frames=16)
    _sweep([("q = 2^-100", ws)], kind, 48000, [Q_FLOOR], "cutoff sweep, filter %d" % kind)
    ws.close()
    good = _sweep_patch(s2.OSC_SAW, kind, 800.0, 3.0, Q_FLOOR)
    bad = _copy_patch(good)
    bad.lpf_q = _pred(Q_FLOOR)
    pr = Pair(16, good, max_frames=64)
    for n in (0, 40, 69, 127):
        pr.note_on(n)
    what = "filter %d at q %s" % (kind, _hx(Q_FLOOR))
    assert_bits_equal_finite(*pr.render_voices(64), what + ", first fill")
    pr.gpu.set_patch(bad)                                       # (the patch itself is in range)
    for call in (lambda: pr.gpu.sample(np.empty(64, dtype=np.float32), 48000), lambda: pr.gpu.render_voices(64, 48000),
                 lambda: pr.gpu.sample_begin(64, 48000), lambda: pr.gpu.sample_stereo(64, 48000)):
        with pytest.raises(s2.S2rError) as e:
            call()
        assert e.value.status == S2R_ERR_PATCH_RANGE, (what, e.value.status)
        assert "lpf.q" in str(e.value), str(e.value)
    pr.gpu.set_patch(good)
    for k in range(2):
        g, w, _ = pr.sample(64)
        assert_bits_equal_finite(g, w, "%s, fill %d after the refusals" % (what, k))
    assert_bits_equal_finite(*pr.render_voices(64), what + ", rows after the refusals")


# ---- f. the border from outside ----

def _outside(lo, hi):
    """the nearest float below lo and above hi (None: unbounded), NaN, +Inf and -Inf"""
    out = [F32(np.nan), F32(np.inf), F32(-np.inf), _pred(lo) if lo != 0.0 else -DENORM_MIN]
    return out + ([_succ(hi)] if hi is not None else [])


REFUSED = ([("lpf_freq", _outside(0.0, None))] +
           [("%s.%s" % (e, t), _outside(0.0, None)) for e in ("amp_env", "mod_env") for t in ("attack_ms", "decay_ms", "release_ms")] +
           [("%s.sustain" % e, _outside(0.0, 1.0)) for e in ("amp_env", "mod_env")] +
           [(k, _outside(-10.0, 10.0)) for k in ("mod_env_to_osc_freq", "mod_env_to_lpf_freq")] +
           [(k, _outside(0.0, 1.0)) for k in ("osc_gain", "noise")] + [(k, _outside(0.0, 10.0)) for k in ("lpf_damping", "lpf_q")])


def test_values_next_to_each_range_are_refused_and_the_handle_renders_on():
    """For every float field of the patch: the nearest float outside its range (-2^-149 below a range that starts at 0), NaN and
    +-Inf are refused by s2r_set_patch and s2r_set_patch_bank with S2R_ERR_PATCH_RANGE (s2r_validate_patch, s2r_patch.cpp:79-99),
    and the next fill of the same handle equals the oracle's with the old patch.  A sample rate of 0 stays S2R_ERR_INVALID
    (check_fill, s2r_host.cpp).  (The borders themselves are rendered by the tests above: -0.0, 0 and FLT_MAX, sustains 0 and
    1, amounts of +-10.)  The MIDI note range has no outside: s2r_note_on takes a u8 like the reference's Note, and notes 128 ..
    255 get note_to_pitch's value (build_pitch_table, s2r_host.cpp, has 256 entries); 128 and 255 are rendered here."""
    good = make_patch(osc_kind=s2.OSC_TRIANGLE, lpf_freq=700.0, mod_env_to_lpf_freq=3.0, mod_env_to_osc_freq=0.5, noise=0.1)
    pr = Pair(16, good, max_frames=64)
    for n in (0, 33, 69, 101, 127):
        pr.note_on(n)
    g, w, _ = pr.sample(48)
    assert_bits_equal_finite(g, w, "before any refusal")
    for field, values in REFUSED:
        for v in values:
            bad = _copy_patch(good)
            if "." in field:
                setattr(getattr(bad, field.split(".")[0]), field.split(".")[1], float(v))
            else:
                setattr(bad, field, float(v))
            what = "%s = %s" % (field, _hx(v))
            for call in (lambda: pr.gpu.set_patch(bad), lambda: pr.gpu.set_patch_bank([good, bad])):
                with pytest.raises(s2.S2rError) as e:
                    call()
                assert e.value.status == S2R_ERR_PATCH_RANGE, (what, e.value.status)
            g, w, _ = pr.sample(48)
            assert_bits_equal_finite(g, w, "the fill after %s was refused" % what)
    for call in (lambda: pr.gpu.sample(np.empty(48, dtype=np.float32), 0), lambda: pr.gpu.render_voices(48, 0),
                 lambda: pr.gpu.sample_begin(48, 0)):
        with pytest.raises(s2.S2rError) as e:
            call()
        assert e.value.status == S2R_ERR_INVALID, e.value.status
    assert_bits_equal_finite(*pr.render_voices(48), "rows after a sample rate of 0 was refused")
    for n in (128, 255):                                        # not a border: Note is a u8 (synth.rs:16) and 440 * 2^((n - 69) / 12) goes on
        v = pr.note_on(n)
        assert_bits_equal_finite(pr.gpu.export_state()["pitch_hz"][v:v + 1], np.array([s2o.lib().s2o_note_to_pitch(n)], dtype=np.float32),
                                 "pitch_hz of note %d" % n)
        assert_bits_equal_finite(*pr.render_voices(48), "rows with note %d sounding" % n)
