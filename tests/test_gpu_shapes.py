"""Parity at the buffer, pool and bank shapes the rest of the suite never builds: a caller's buffer of any length (441, 480,
1000 ... frames, max_frames that are no multiple of 16 or of 4, fills past 64 Ki frames), pools with more workgroups than
the device has compute units, banks of up to S2R_MAX_BANK patches, and coefficient tables near S2R_TAB_MAX_ENTRIES and
the bank's 2^28-float budget.  Every check is bit for bit against the oracle (helpers.Pair, s2o.mix_tree /
mix_tree_partial), driven as the reference's caller drives Synth: events applied between 16-frame sample() calls
(s2_bin/src/main.rs:138-147).  The shape-dependent sites each test reaches are named in its docstring."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import Pair, assert_bits_equal, make_patch, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2

pytestmark = pytest.mark.gpu
SR = 48000
SUPER_WHOLE = 1024                  # kSuperWhole (s2r_kern_common.h): the longest fill rendered as one super-chunk
EVENT_FRAME_MAX = 65520             # the last 16-aligned frame a 16-bit s2r_note_event.frame can name
TAB_MAX = 1 << 22                   # S2R_TAB_MAX_ENTRIES (s2r_device.h)


def _threads():
    return max(1, min(32, len(os.sched_getaffinity(0))))


def _onepole_patch():
    p = make_patch(osc_kind=s2.OSC_SAW, noise=0.1, mod_env_to_lpf_freq=3.0, lpf_freq=700.0)
    p.amp_env.attack_ms = 2.0; p.amp_env.decay_ms = 15.0; p.amp_env.release_ms = 10.0
    p.mod_env.attack_ms = 1.0; p.mod_env.decay_ms = 12.0; p.mod_env.sustain = 0.3; p.mod_env.release_ms = 8.0
    return p


def _general_patch(kind=s2.FILT_SVF_LP):
    p = make_patch(osc_kind=s2.OSC_TRIANGLE, lpf_kind=kind, lpf_freq=1200.0, lpf_q=1.7, lpf_damping=0.8, mod_env_to_osc_freq=0.6,
                   mod_env_to_lpf_freq=2.0, noise=0.05)
    p.amp_env.attack_ms = 3.0; p.amp_env.decay_ms = 20.0; p.amp_env.release_ms = 12.0
    p.mod_env.attack_ms = 2.0; p.mod_env.decay_ms = 10.0; p.mod_env.sustain = 0.4; p.mod_env.release_ms = 6.0
    return p


def _small_bank():
    return [_onepole_patch(), make_patch(osc_kind=s2.OSC_SINE, lpf_kind=s2.FILT_LP2, lpf_freq=900.0, noise=0.2),
            make_patch(osc_kind=s2.OSC_DPW_SAW, lpf_kind=s2.FILT_SVF_LP, lpf_q=1.3),
            make_patch(osc_kind=s2.OSC_DPW_SQUARE, lpf_kind=s2.FILT_HP2, lpf_damping=0.9, mod_env_to_osc_freq=0.4)]


def _pair(kind, voices, max_frames, block=0, groups=0):
    """a Pair whose handle renders with the one-pole kernel, the general kernel (SVF + oscillator FM) or the bank kernel"""
    if kind == "bank":
        pr = Pair(voices, max_frames=max_frames, block_voices=block, mix_groups=groups)
        pr.set_bank(_small_bank())
        pr.bank_size = 4
    else:
        pr = Pair(voices, _onepole_patch() if kind == "onepole" else _general_patch(), max_frames=max_frames, block_voices=block,
                  mix_groups=groups)
        pr.bank_size = 1
    pr.threads = _threads()
    return pr


def _events(rng, frames, n, bank_size=1, timed=True, first_on=None):
    """a batch of note events for a fill of `frames`: times on the 16-frame grid, sorted; program changes among them for a
    bank; timed batches always hold an event at the fill's last 16-aligned frame and, in a fill that reaches it, at frame
    65 520 (the last a 16-bit frame can name)"""
    rows = []
    if first_on:
        rows += [(1, 30 + (k * 7) % 70, 0, 1.0) for k in range(first_on)]
    reach = min(frames, EVENT_FRAME_MAX + 1)                 # (a fill past 65 536 frames takes events up to 65 520 only)
    times = sorted(int(t) * 16 for t in rng.randint(0, (reach + 15) // 16, n)) if timed else [0] * n
    if timed:
        times.append((reach - 1) // 16 * 16)
        if frames > EVENT_FRAME_MAX:
            times.append(EVENT_FRAME_MAX)
        times.sort()
    for t in times:
        if bank_size > 1 and rng.rand() < 0.3:
            rows.append((2, int(rng.randint(bank_size)), t, 0.0))
        rows.append((int(rng.rand() < 0.6), int(rng.randint(30, 100)), t, 1.0))
    return np.array(rows, dtype=s2.NOTE_EVENT_DTYPE) if rows else np.zeros(0, dtype=s2.NOTE_EVENT_DTYPE)


def _oracle_rows(pr, ev, frames, sr=SR):
    with np.errstate(all="ignore"):
        return pr.cpu.render_events(ev, frames, sr, threads=pr.threads)


def _lengths(max_frames):
    """1, 15, 16, 17, max_frames - 1, max_frames and one length on each side of the one-super-chunk threshold"""
    return sorted({n for n in (1, 15, 16, 17, max_frames - 1, max_frames, SUPER_WHOLE, SUPER_WHOLE + 1) if 1 <= n <= max_frames})


class _Ring:
    """s2r_fill_begin / s2r_fill_end with two fills in flight, every buffer against the oracle's mix"""

    def __init__(self, pr, what):
        self.pr, self.what, self.queue = pr, what, []

    def begin(self, ev, frames, tag):
        self.pr.gpu.note_events(ev)
        self.pr.gpu.sample_begin(frames, SR)
        self.queue.append((tag, frames, s2o.mix_tree(_oracle_rows(self.pr, ev, frames), self.pr.block_voices, self.pr.groups)))
        if len(self.queue) == 2:
            self.end()

    def end(self):
        tag, frames, want = self.queue.pop(0)
        assert_bits_equal(self.pr.gpu.sample_end(np.empty(frames, dtype=np.float32)), want, "%s, %s (ring)" % (self.what, tag))

    def drain(self):
        while self.queue:
            self.end()


def _fill(pr, form, ev, frames, what):
    """one fill of `frames` in the given form (the events `ev` handed over first), against the oracle"""
    pr.gpu.note_events(ev)
    if form == "sample":
        got = pr.gpu.sample(np.empty(frames, dtype=np.float32), SR)
        assert_bits_equal(got, s2o.mix_tree(_oracle_rows(pr, ev, frames), pr.block_voices, pr.groups), what + " (sample)")
    elif form == "stereo":
        lr = pr.gpu.sample_stereo(frames, SR)
        want = s2o.mix_tree(_oracle_rows(pr, ev, frames), pr.block_voices, pr.groups)
        assert_bits_equal(lr[:, 0], want, what + " (stereo, left)")
        assert_bits_equal(lr[:, 1], want, what + " (stereo, right)")
    elif form == "voices":
        assert_bits_equal(pr.gpu.render_voices(frames, SR), _oracle_rows(pr, ev, frames), what + " (per-voice rows)")
    else:
        raise ValueError(form)


def _oversampled(pr, rng, lengths, what):
    """s2r_fill_oversampled at the given lengths, untimed events between the calls, the 63-tap decimator's history carried
    from call to call (it starts at zero on a fresh handle)"""
    hist = np.zeros(62, dtype=np.float32)
    for k, n in enumerate(lengths):
        ev = _events(rng, 4 * n, 3, pr.bank_size, timed=False)
        pr.gpu.note_events(ev)
        got = pr.gpu.sample_oversampled(n, SR)
        x = np.concatenate([hist, s2o.mix_tree(_oracle_rows(pr, ev, 4 * n, 4 * SR), pr.block_voices, pr.groups)])
        hist = x[-62:]
        assert_bits_equal(got, s2o.decimate4(x, n), "%s, oversampled call %d (%d frames)" % (what, k, n))


def _oracle_layer_rows(bank, layers, frames):
    """the oracle's process_layer_buf_simd (process.rs:14-49) per layer: rows and the layers' states afterwards"""
    L = s2o.lib()
    rows = np.zeros((layers.size, frames), dtype=np.float32)
    after = layers.copy()
    for i in range(layers.size):
        c = layers[i]
        cfg = oracle_cfg_from_patch(bank[int(c["program"])])
        st = s2o.LayerState()
        st.has_phase = 1; st.phase_accum = float(c["phase_accum"]); st.seed = int(c["noise_seed"]); st.lpf_last = float(c["lpf_last"])
        st.x1, st.x2, st.y1, st.y2 = (float(c[k]) for k in ("filt_x1", "filt_x2", "filt_y1", "filt_y2"))
        z = float(c["osc_z"])
        st.has_z = 0 if np.isnan(z) else 1
        st.dpw_z = 0.0 if np.isnan(z) else z
        with np.errstate(all="ignore"):
            assert L.s2o_process_layer_buf_simd(C.byref(cfg), C.byref(st), float(c["pitch_hz"]), SR, int(c["offset"]),
                                                int(c["has_release"]), int(c["release_offset"]), s2o._fp(rows[i]), frames) == 0
        after[i]["phase_accum"] = st.phase_accum; after[i]["lpf_last"] = st.lpf_last
        after[i]["filt_x1"], after[i]["filt_x2"], after[i]["filt_y1"], after[i]["filt_y2"] = st.x1, st.x2, st.y1, st.y2
        after[i]["osc_z"] = st.dpw_z if st.has_z else np.float32(np.nan)
    return rows, after


def _process_layers(kind, rng, max_frames, lengths, what):
    """s2r_process_layers on a workspace handle of `max_frames`, the layers' states carried from call to call"""
    bank = _small_bank() if kind == "bank" else [_onepole_patch() if kind == "onepole" else _general_patch()]
    ws = s2.Synth(96, max_frames=max_frames, block_voices=64)
    if len(bank) > 1:
        ws.set_patch_bank(bank)
    else:
        ws.set_patch(bank[0])
    n = 70
    layers = np.zeros(n, dtype=s2.LAYER_CALL_DTYPE)
    layers["pitch_hz"] = np.exp(rng.uniform(np.log(30.0), np.log(5000.0), n)).astype(np.float32)
    layers["offset"] = rng.randint(0, 3000, n)                         # offsets of every residue mod 16
    rel = rng.rand(n) < 0.3
    layers["has_release"] = rel
    layers["release_offset"] = np.where(rel, (layers["offset"] * rng.rand(n)).astype(np.uint32), 0)
    layers["program"] = rng.randint(0, len(bank), n)
    layers["noise_seed"] = rng.randint(0, 1 << 31, n)
    layers["osc_z"] = np.float32(np.nan)
    for k, frames in enumerate(lengths):
        want, after = _oracle_layer_rows(bank, layers, frames)
        got = ws.process_layers(layers, frames, SR)
        assert_bits_equal(got, want, "%s, process_layers call %d (%d frames)" % (what, k, frames))
        for f in ("phase_accum", "lpf_last", "filt_x1", "filt_x2", "filt_y1", "filt_y2", "osc_z"):
            assert_bits_equal(layers[f], after[f], "%s, process_layers call %d: %s" % (what, k, f))
        layers["offset"] += frames
    ws.close()


def _assert_state_is_the_oracle_s(pr, what):
    """the handle's exported voice state equals the oracle's voice by voice, bit for bit"""
    st = pr.gpu.export_state()
    for i in range(pr.cpu.num_voices):
        v = pr.cpu.voice(i)
        if not v.has_current:
            assert not st["started"][i], "%s: voice %d started on the GPU only" % (what, i)
            continue
        assert st["current_frame_offset"][i] == v.current_frame_offset, "%s: voice %d offset" % (what, i)
        assert bool(st["released"][i]) == bool(v.has_release), "%s: voice %d released" % (what, i)
        for name, a, b in (("phase", st["phase_accum"][i], v.state.phase_accum), ("x1", st["filt_x1"][i], v.state.x1),
                           ("x2", st["filt_x2"][i], v.state.x2), ("y1", st["filt_y1"][i], v.state.y1), ("y2", st["filt_y2"][i], v.state.y2),
                           ("lpf_last", st["lpf_last"][i], v.state.lpf_last)):
            assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), "%s: voice %d %s" % (what, i, name)


def _assert_resident(pr, what):
    """one more 16-frame fill with the pool-resident kernel's state read at once (it leaves after 2 ms without a command, and the
    oracle's share of a fill may take longer), then the fill checked against the oracle"""
    got = pr.gpu.sample(np.empty(16, dtype=np.float32), SR)
    active = pr.gpu.resident_active
    assert_bits_equal(got, s2o.mix_tree(_oracle_rows(pr, np.zeros(0, dtype=s2.NOTE_EVENT_DTYPE), 16), pr.block_voices, pr.groups),
                      what + ", last fill")
    assert active, "%s: the pool-resident kernel did not take the last fill" % what


# ---- 1. buffer lengths, every fill form ----

LONG_FRAMES = 70001


@pytest.mark.parametrize("max_frames", [1, 17, 441, 1000, 1023, 1025, 3001, 8192, LONG_FRAMES])
@pytest.mark.parametrize("kind", ["onepole", "general", "bank"])
def test_buffer_lengths_every_fill_form(kind, max_frames):
    """A caller's buffer of any length, through every form a handle offers (sample, two begun fills in flight, stereo, per-voice
    rows, 4x oversampled, process_layers), for both render kernels and the bank kernel; 70 voices in 64-voice workgroups (a
    ragged second one).  Sites: the partial rows' stride rounded up to 4 (partials_stride, s2r_host.cpp) and the row zeroing
    that stops at (frames + 3) & ~3 (s2r_render_onepole.inc:92, s2r_render_general.inc:308) at max_frames that are no
    multiple of 4; the one-super-chunk threshold on both sides (s2r_pick_super_frames, s2r_kern_common.h:746-755); offsets
    that are no multiple of 16 leaving the branch-free chunk (s2r_render_onepole.inc:461); timed events at a fill's last
    16-aligned frame and at frame 65 520 (the 16-bit S2rPolicyEvent frame, s2r_voices.h:126).  Catches a stride, a tail or a
    zeroing bound off by one, and an event frame truncated or mis-scaled."""
    rng = np.random.RandomState(max_frames * 3 + len(kind))
    voices = 70 if max_frames < LONG_FRAMES else 40
    pr = _pair(kind, voices, max_frames, block=64)
    what = "%s, max_frames %d" % (kind, max_frames)
    lens = _lengths(max_frames)
    ring = _Ring(pr, what)
    # the pool first: every voice sounding, so the ragged workgroup has voices in it
    _fill(pr, "sample", _events(rng, lens[0], 4, pr.bank_size, first_on=voices), lens[0], what + ", pool filled")
    for form in ("sample", "ring", "stereo", "voices"):
        for n in (lens if form != "ring" else lens + lens[::-1]):
            ev = _events(rng, n, int(rng.randint(1, 12)), pr.bank_size, timed=form != "voices" and rng.rand() < 0.7)
            if form == "ring":
                ring.begin(ev, n, "%d frames" % n)
            else:
                ring.drain()
                _fill(pr, form, ev, n, "%s, %d frames" % (what, n))
        ring.drain()
    # 4x oversampled: 4 * frames <= max_frames, and 4 * frames no multiple of 16 where the size allows one
    q = max_frames // 4
    if q:
        _oversampled(pr, rng, sorted({n for n in (1, 3, 5, 17, q - 1, q) if 1 <= n <= q}, reverse=True), what)
    _process_layers(kind, rng, max_frames, [n for n in lens if n <= 8192] + [lens[0]], what)
    _assert_state_is_the_oracle_s(pr, what)


# ---- 2. the resident forms at these lengths ----

@pytest.mark.parametrize("max_frames", [441, 1023, 3001, LONG_FRAMES])
@pytest.mark.parametrize("kind", ["onepole", "general", "bank"])
def test_pool_resident_kernel_at_odd_lengths(kind, max_frames):
    """s2r_set_resident on a pool of eight (70001: two) 64-voice workgroups: fills that alternate between short ones and
    max_frames, ring and synchronous, timed events at the last 16-aligned frame and at 65 520; at 70 001 frames the fills
    cross the pool-resident limit of 0xffff frames (pool_eligible, s2r_host.cpp) both ways on one handle.  Sites: the
    resident kernel's LDS and staging sized from max_frames, not from the fill (pool_launch, s2r_host.cpp); the super-chunk choice per
    fill (s2r_kern_common.h:746-755); the partial-row stride (s2r_host.cpp).  Catches staging sized or indexed by the wrong
    length, a form switch that loses or repeats state, and a fill length carried over from the previous command.  The exported
    state is compared with the oracle's at the end."""
    rng = np.random.RandomState(1000 + max_frames + len(kind))
    voices = 512 if max_frames < LONG_FRAMES else 128
    pr = _pair(kind, voices, max_frames, block=64)
    pr.gpu.set_resident(True)
    what = "resident, %s, max_frames %d" % (kind, max_frames)
    ring = _Ring(pr, what)
    if max_frames < LONG_FRAMES:
        lens = [max_frames, 17, max_frames, 1, max_frames - 1, 16, min(SUPER_WHOLE + 1, max_frames), max_frames, 15, max_frames]
    else:
        lens = [65535, max_frames, 17, 65536, 65535, 1025, max_frames - 1, 1000]
    for k, n in enumerate(lens):
        ev = _events(rng, n, int(rng.randint(0, 40)), pr.bank_size, timed=k > 0, first_on=voices if k == 0 else None)
        if k % 3 == 2:
            ring.drain()
            _fill(pr, "sample", ev, n, "%s, fill %d (%d frames)" % (what, k, n))
        else:
            ring.begin(ev, n, "fill %d (%d frames)" % (k, n))
    ring.drain()
    _assert_resident(pr, what)
    _assert_state_is_the_oracle_s(pr, what)


@pytest.mark.parametrize("max_frames", [441, 1023])
def test_low_latency_kernel_at_odd_lengths(max_frames):
    """s2r_set_low_latency on a pool of one workgroup (60 voices, a one-pole patch) at max_frames that are no multiple of 16 or 4:
    the reference's 16-frame calls, ragged calls of 1, 15 and 17 frames, and whole buffers.  Sites: the resident kernel's
    staging sized from max_frames (pool_launch and resident_launch, s2r_host.cpp), the row zeroing at (frames + 3) & ~3 (s2r_render_onepole.inc:92), the
    tail past the last whole chunk.  Catches a tail or a bound that assumes max_frames a multiple of 16."""
    rng = np.random.RandomState(max_frames)
    pr = _pair("onepole", 60, max_frames)
    pr.gpu.set_low_latency(True)
    what = "low latency, max_frames %d" % max_frames
    lens = [16, 16, 1, 15, 17, 16, max_frames, 16, max_frames - 1, 32, 16, 17]
    active = 0
    for k, n in enumerate(lens * 2):
        ev = _events(rng, n, int(rng.randint(0, 4)), timed=False, first_on=50 if k == 0 else None)
        pr.gpu.note_events(ev)
        got = pr.gpu.sample_stereo(n, SR) if k % 7 == 3 else pr.gpu.sample(np.empty(n, dtype=np.float32), SR)
        active += int(pr.gpu.low_latency_active)             # (read before the oracle's share: the kernel leaves when idle)
        want = s2o.mix_tree(_oracle_rows(pr, ev, n), pr.block_voices, pr.groups)
        for col in ([0, 1] if got.ndim == 2 else [None]):
            assert_bits_equal(got if col is None else got[:, col], want, "%s, fill %d (%d frames)" % (what, k, n))
    assert active >= len(lens), (what, active)
    _assert_state_is_the_oracle_s(pr, what)


# ---- 3. device lists at odd max_frames ----

@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("interleave", [0, 16, 64])
@pytest.mark.parametrize("max_frames", [1000, 1023])
@pytest.mark.parametrize("n", [2, 3])
def test_device_list_exchange_at_odd_max_frames(n, max_frames, interleave, resident):
    """A device list of n shards on one card at max_frames 1000 and 1023: the shards' rows go through the root's exchange rows,
    laid out at a stride of max_frames itself, unrounded (pool_launch, enqueue_multi and enqueue_root, s2r_host.cpp; read at
    s2r_kern_common.h:1171) — at 1023 a stride that is no multiple of 4.  Ring and synchronous fills of max_frames, 17 and
    max_frames - 1 frames, contiguous shards or runs of 16 / 64 voices dealt out, launch per fill or resident.  Expects the
    rank-ordered sum of the shards' trees over the oracle's rows.  Catches a writer and a reader of the exchange rows that
    disagree on the stride or on a shard's row."""
    rng = np.random.RandomState(n * 100 + max_frames + interleave + int(resident))
    V = 768
    multi = s2.Synth(V, max_frames=max_frames, devices=[0] * n, shard_interleave=interleave, block_voices=64)
    if resident:
        multi.set_resident(True)
    ora = s2o.OracleSynth(V)
    what = "device list of %d, max_frames %d, interleave %d, resident %d" % (n, max_frames, interleave, resident)

    def want_of(ev, frames):
        with np.errstate(all="ignore"):
            pv = ora.render_events(ev, frames, SR, threads=_threads())
        acc = np.zeros(frames, dtype=np.float32)
        for k in range(n):
            idx = s2.shard_pool_indices(V, k, n, interleave) if interleave else np.arange(k * V // n, (k + 1) * V // n)
            acc = acc + s2o.mix_tree_partial(pv[idx], multi.block_voices)
        return acc

    queue = []
    lens = [max_frames, max_frames, 17, max_frames - 1, max_frames, 1, max_frames]
    for k, frames in enumerate(lens):
        ev = _events(rng, frames, int(rng.randint(0, 200)), timed=k > 0, first_on=V if k == 0 else None)
        multi.note_events(ev)
        multi.sample_begin(frames, SR)
        queue.append((k, frames, want_of(ev, frames)))
        if len(queue) == 2:
            kk, ff, w = queue.pop(0)
            assert_bits_equal(multi.sample_end(np.empty(ff, dtype=np.float32)), w, "%s, ring buffer %d" % (what, kk))
    while queue:
        kk, ff, w = queue.pop(0)
        assert_bits_equal(multi.sample_end(np.empty(ff, dtype=np.float32)), w, "%s, ring buffer %d" % (what, kk))
    for k, frames in enumerate([max_frames, 17, max_frames - 1]):
        ev = _events(rng, frames, 60, timed=True)
        multi.note_events(ev)
        got = multi.sample(np.empty(frames, dtype=np.float32), SR).copy()
        assert_bits_equal(got, want_of(ev, frames), "%s, s2r_fill %d (%d frames)" % (what, k, frames))
    got = multi.sample(np.empty(16, dtype=np.float32), SR).copy()
    active = multi.resident_active                           # (read at once: the kernel leaves after 2 ms without a command)
    assert_bits_equal(got, want_of(np.zeros(0, dtype=s2.NOTE_EVENT_DTYPE), 16), "%s, last fill" % what)
    assert active == resident
    multi.close()


# ---- 4. pools with more workgroups than compute units ----

@pytest.mark.parametrize("kind,voices,block,lens", [
    ("onepole", 16450, 64, (1024, 1025, 4097)),          # 258 workgroups: more than the 256 CUs, the last one with 2 voices
    ("general", 16450, 64, (1024, 1025, 4097)),
    ("onepole", 4100, 256, (1024, 1025, 4097)),          # 17 workgroups: one super-chunk at 1024, 256-frame ones past it
    ("onepole", 4100, 512, (1024, 1025, 4097)),          # 64-frame super-chunks
    ("onepole", 4100, 1024, (1024, 1025, 4097)),         # 32-frame super-chunks
    ("bank", 4100, 512, (1024, 4097)),
    ("onepole", 66001, 64, (1024, 1025)),                # 1032 workgroups
])
def test_pool_with_more_workgroups_than_compute_units(kind, voices, block, lens):
    """Pools whose voice count is no multiple of 64, in workgroups of 64 to 1024 voices, with mix_groups 3: grids with more
    workgroups than the device has compute units, where s2r_pick_super_frames (s2r_kern_common.h:746-755) leaves the
    one-super-chunk layout for 256-, 64- and 32-frame super-chunks in two LDS buffers, and the last workgroup is ragged.  Fills of
    1024, 1025 and 4097 frames with timed events.  Catches a super-chunk loop or a group-sum buffer off by one at a ragged
    fill, a ragged workgroup's lanes summed into the mix, and a group boundary of the three-group tree in the wrong place.
    Found: the one-launch mix (mix_block, s2r_kern_common.h:986-1031, called by fused_tail) added up only 16 x (threads / 16)
    of the runs of 16 workgroups in 64-voice workgroups — below."""
    rng = np.random.RandomState(voices + block + len(kind))
    pr = _pair(kind, voices, max(lens), block=block, groups=3)
    what = "%s, %d voices, block %d, 3 groups" % (kind, voices, block)
    for k, n in enumerate(lens):                          # (the first fill's batch starts every voice of the pool)
        _fill(pr, "sample", _events(rng, n, 300, pr.bank_size, first_on=voices if k == 0 else None), n, "%s, %d frames" % (what, n))


@pytest.mark.parametrize("voices,block,groups", [(4100, 64, 1), (4100, 64, 3), (16500, 128, 1)])
def test_one_launch_mix_with_more_runs_than_a_small_workgroup_has_slots(voices, block, groups):
    """Regression (found by the test above): in the one-launch form the last workgroups to finish add the partial rows up in
    runs of 16 workgroups (mix_block, s2r_kern_common.h:986-1031, called by fused_tail); its threads stepped through the runs by
    16 slots, as many as a 256-thread workgroup has, so a 64-voice workgroup (4 slots) or a 128-voice one (8) skipped every run
    past its own slots and added whatever its LDS held instead.  Pools of more than 64 workgroups of 64 voices, or 128 of 128,
    one or three mix groups, synchronous and ring fills."""
    rng = np.random.RandomState(voices + block + groups)
    pr = _pair("onepole", voices, 1024, block=block, groups=groups)
    what = "one-launch mix, %d voices, block %d, %d groups" % (voices, block, groups)
    _fill(pr, "sample", _events(rng, 1024, 100, first_on=voices), 1024, what + ", sync")
    ring = _Ring(pr, what)
    for k, n in enumerate((1024, 1000, 1024)):
        ring.begin(_events(rng, n, 100), n, "ring %d" % k)
    ring.drain()


# ---- 5. bank and table edges ----

def _bank256():
    """256 distinct patches: every oscillator kind (the DPW shapes included) and every filter kind, short envelopes"""
    bank = []
    for i in range(256):
        p = make_patch(osc_kind=i % 7, lpf_kind=(i // 7) % 9, osc_gain=1.0 - (i % 11) * 0.05, noise=0.02 * (i % 5),
                       lpf_freq=200.0 + 37.0 * i, mod_env_to_lpf_freq=(i % 9) * 0.5 - 1.0, mod_env_to_osc_freq=0.3 * (i % 3) - 0.3,
                       lpf_damping=0.5 + 0.01 * i, lpf_q=0.7 + 0.02 * i)
        p.amp_env.attack_ms = 1.0 + (i % 4); p.amp_env.decay_ms = 5.0 + (i % 13); p.amp_env.release_ms = 4.0 + (i % 6)
        p.mod_env.attack_ms = (i % 3) * 1.5; p.mod_env.decay_ms = 3.0 + (i % 17); p.mod_env.sustain = (i % 10) * 0.1
        p.mod_env.release_ms = 2.0 + (i % 8)
        bank.append(p)
    return bank


@pytest.mark.parametrize("resident", [False, True])
def test_bank_of_256_patches(resident):
    """A bank of S2R_MAX_BANK distinct patches (every oscillator kind, DPW included, every filter kind), voices on programs 0,
    1, 254 and 255 and on the rest, program changes inside timed event batches; launch per fill: per-voice rows after untimed
    batches (s2r_render_voices takes no timed events) and mixes after timed ones; pool-resident: ring and synchronous mixes;
    then the exported state.  Site: ensure_bank (s2r_host.cpp) packing 256 patches'
    four table planes at tab_off, the last patch's table ending the buffer.  Catches a patch read from or tabulated for a
    neighbour's entry, a tab_off past patch 7, and a program index truncated below 8 bits."""
    rng = np.random.RandomState(256 + int(resident))
    bank = _bank256()
    voices = 300
    pr = Pair(voices, max_frames=1024, block_voices=64)
    pr.set_bank(bank)
    pr.bank_size, pr.threads = 256, _threads()
    if resident:
        pr.gpu.set_resident(True)
    what = "bank of 256, resident %d" % resident
    rows = []
    for v in range(voices):                                  # programs 0, 1, 254, 255 first, then every program
        rows.append((2, (0, 1, 254, 255)[v % 4] if v < 64 else v % 256, 0, 0.0))
        rows.append((1, 30 + (v * 7) % 70, 0, 1.0))
    ev0 = np.array(rows, dtype=s2.NOTE_EVENT_DTYPE)
    ring = _Ring(pr, what)
    for k in range(8):
        frames = (1024, 1000, 17, 1024, 441, 1024, 1023, 1024)[k]
        ev = ev0 if k == 0 else _events(rng, frames, 80, 256, timed=resident or k % 2 == 1)
        if k:
            pc = ev["kind"] == 2
            ev["note"][pc] = rng.choice([0, 1, 254, 255, 128, 7], int(pc.sum()))
        if not resident:
            _fill(pr, "voices" if k % 2 == 0 else "sample", ev, frames, "%s, fill %d (%d frames)" % (what, k, frames))
        elif k % 3 == 2:
            ring.drain()
            _fill(pr, "sample", ev, frames, "%s, fill %d (%d frames)" % (what, k, frames))
        else:
            ring.begin(ev, frames, "fill %d (%d frames)" % (k, frames))
        if k == 0:
            ring.drain()
            assert list(pr.gpu.export_state()["program"][:8]) == [0, 1, 254, 255] * 2
    ring.drain()
    if resident:
        _assert_resident(pr, what)
    _assert_state_is_the_oracle_s(pr, what)


def _ms_as_samples(ms):
    return np.float32(s2o.lib().s2o_ms_as_samples(float(ms), SR))


def _ms_at_cut(base_samples, below):
    """the decay (or release) time in ms for which base_samples + Ms::as_samples(ms) (f32, units.rs:44-53) is the largest
    value below S2R_TAB_MAX_ENTRIES (below) or the smallest at or past it"""
    ms = np.float32((TAB_MAX - float(base_samples)) * 1000.0 / SR)
    up, down = np.float32(1e9), np.float32(0)
    while np.float32(base_samples) + _ms_as_samples(ms) < TAB_MAX:
        ms = np.nextafter(ms, up)
    while np.float32(base_samples) + _ms_as_samples(ms) >= TAB_MAX:
        ms = np.nextafter(ms, down)
    return float(ms) if below else float(np.nextafter(ms, up))


def _edge_patch(below, osc=s2.OSC_SAW, kind=s2.FILT_LP2, fm=0.5):
    """a patch whose mod envelope reaches sustain (attack + decay) and ends its release just below S2R_TAB_MAX_ENTRIES frames
    (tabulated) or at it (computed in-lane: plan_tables, s2r_host.cpp), asserted with the oracle's Ms::as_samples;
    the amp envelope's release twice as long, so that the filter coefficients stay audible through the whole release"""
    p = make_patch(osc_kind=osc, lpf_kind=kind, lpf_freq=800.0, lpf_damping=0.7, lpf_q=1.4, mod_env_to_lpf_freq=3.0,
                   mod_env_to_osc_freq=fm, noise=0.05)
    p.mod_env.attack_ms = 1.0
    A = _ms_as_samples(1.0)
    p.mod_env.decay_ms = _ms_at_cut(A, below)
    p.mod_env.sustain = 0.3
    p.mod_env.release_ms = _ms_at_cut(0.0, below)
    sus_off = A + _ms_as_samples(p.mod_env.decay_ms)
    R = _ms_as_samples(p.mod_env.release_ms)
    assert (sus_off < TAB_MAX and R < TAB_MAX) if below else (sus_off >= TAB_MAX and R >= TAB_MAX), (sus_off, R)
    p.amp_env.attack_ms = 1.0; p.amp_env.decay_ms = 5.0; p.amp_env.sustain = 0.8; p.amp_env.release_ms = 2.0 * p.mod_env.release_ms
    return p


def _age_to_region_ends(pr, patch, voices):
    """Puts `voices` (started with `patch`) within one chunk of every end of its table regions (S2rTabRef, s2r_device.h):
    attack + decay -> sustain (ad), the end of a release from the clamp (rc), the end of a later release (ru) — 32 consecutive
    offsets each, every residue mod 16, on both sides of the boundary; the oracle's voices get the same edit."""
    A = _ms_as_samples(patch.mod_env.attack_ms)
    sus_off = A + _ms_as_samples(patch.mod_env.decay_ms)
    R = _ms_as_samples(patch.mod_env.release_ms)
    rc_t0 = int(np.ceil(float(sus_off)))
    r_end = int(np.ceil(float(R)))
    st = pr.gpu.export_state()
    for j, v in enumerate(voices):
        which, k = j % 3, (j // 3) % 32 - 20                  # k: the chunk before the boundary, the one across it, the one after
        if which == 0:                                        # ad -> sustain, never released
            t, rel = rc_t0 + k, None
        elif which == 1:                                      # released in the decay: the release runs from the clamp (rc)
            t, rel = rc_t0 + r_end + k, rc_t0 // 2
        else:                                                 # released in sustain (ru)
            rel = rc_t0 + 5000
            t = rel + r_end + k
        st["current_frame_offset"][v] = t
        pr.cpu.voice(int(v)).current_frame_offset = t
        st["released"][v] = 0 if rel is None else 1
        st["release_frame_offset"][v] = 0 if rel is None else rel
        pr.cpu.voice(int(v)).has_release = 0 if rel is None else 1
        pr.cpu.voice(int(v)).release_frame_offset = 0 if rel is None else rel
    pr.gpu.import_state(st)


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("case", ["single_onepole", "single_general", "bank_last", "over_budget"])
def test_table_region_edges(case, resident):
    """Voices aged by export_state / import_state (as test_gpu_fuzz does) to within one chunk of the ends of their coefficient
    tables' regions (ad -> sus, rc -> end, ru -> end; lanes without a voice read `dead`), at every residue mod 16, for patches
    whose mod envelope sits just below S2R_TAB_MAX_ENTRIES frames: the single-patch table (one-pole and general kernels), the
    last patch of a bank — its table ends the bank's buffer, next to a patch at the limit that computes in-lane — and a bank of
    six such patches that passes the 2^28-float budget, so that the sixth computes in-lane beside five tabled ones in one wave
    (this allocates about 1 GiB of tables).  Sites: plan_tables (s2r_host.cpp: the cut and the regions' lengths),
    ensure_bank (s2r_host.cpp: tab_off and the budget), the chunk's reads up to S2R_TAB_PAD entries past a region's last
    used entry (s2r_device.h:97).  Catches a region one entry short, a pad read from the next region or past the buffer, the
    cut on the wrong side, and tabled and in-lane lanes of one wave mixed up."""
    voices = 640 if case == "over_budget" else 256
    if case.startswith("single"):
        patch = _edge_patch(True, osc=s2.OSC_SINE, kind=s2.FILT_ONEPOLE if case == "single_onepole" else s2.FILT_LP2,
                            fm=0.0 if case == "single_onepole" else 0.5)
        bank = [patch]
    elif case == "bank_last":
        bank = [_onepole_patch(), _general_patch(), _edge_patch(False, osc=s2.OSC_DPW_SAW, kind=s2.FILT_SVF_LP),
                _edge_patch(True, osc=s2.OSC_SQUARE, kind=s2.FILT_BP2)]
    else:
        kinds = [(s2.OSC_SAW, s2.FILT_ONEPOLE), (s2.OSC_SINE, s2.FILT_LP2), (s2.OSC_TRIANGLE, s2.FILT_HP1),
                 (s2.OSC_DPW_SQUARE, s2.FILT_SVF_BP), (s2.OSC_SQUARE, s2.FILT_HP2), (s2.OSC_DPW_TRIANGLE, s2.FILT_LP1)]
        bank = [_edge_patch(True, osc=o, kind=f, fm=0.25 * (i % 3)) for i, (o, f) in enumerate(kinds)]
    pr = Pair(voices, bank[0] if len(bank) == 1 else None, max_frames=1024, block_voices=64)
    if len(bank) > 1:
        pr.set_bank(bank)
    pr.bank_size, pr.threads = len(bank), _threads()
    if resident:
        pr.gpu.set_resident(True)
    what = "table edges, %s, resident %d" % (case, resident)
    # programs: the bank's last patch on most voices (bank_last), every patch in turn in each wave (over_budget); 40 lanes idle
    rows = []
    used = voices - 40
    for v in range(used):
        if len(bank) > 1:
            rows.append((2, len(bank) - 1 if case == "bank_last" and v % 4 else v % len(bank), 0, 0.0))
        rows.append((1, 30 + (v * 5) % 70, 0, 1.0))
    _fill(pr, "sample", np.array(rows, dtype=s2.NOTE_EVENT_DTYPE), 64, what + ", started")
    for v in range(used):                                    # the same note_on order gives the same voices on both sides
        assert pr.cpu.voice(v).has_current
    for p in range(len(bank)):
        _age_to_region_ends(pr, bank[p], [v for v in range(used) if len(bank) == 1 or pr.cpu.voice(v).program == p])
    ring = _Ring(pr, what)
    ev = np.zeros(0, dtype=s2.NOTE_EVENT_DTYPE)              # (no note_on: it would steal the oldest voices, the aged ones)
    for k, frames in enumerate((48, 33, 64, 16, 47)):
        if not resident:
            _fill(pr, "voices", ev, frames, "%s, fill %d (%d frames)" % (what, k, frames))
        elif k % 2:
            ring.begin(ev, frames, "fill %d (%d frames)" % (k, frames))
        else:
            ring.drain()
            _fill(pr, "sample", ev, frames, "%s, fill %d (%d frames)" % (what, k, frames))
    ring.drain()
    if resident:
        _assert_resident(pr, what)
    _assert_state_is_the_oracle_s(pr, what)


# ---- 6. the shape fuzzer ----

FUZZ_MAX_FRAMES = [1, 7, 17, 100, 441, 480, 512, 1000, 1023, 1025, 1040, 1500, 2047, 3001, 4097, 8192]


# S2R_FUZZ_SEEDS=N widens the sweep (N / 4 cases), S2R_FUZZ_BASE moves it, like the other fuzzers; its own RandomState stream,
# so test_fuzz's seeds still name the cases they named
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("S2R_FUZZ_SEEDS", "40")) // 4)))
def test_fuzz_shapes(seed):
    """Random buffer shapes: max_frames mostly no multiple of 16, a fill form per buffer (sample, a begun fill, stereo, per-voice
    rows, 4x oversampled), block size, a bank of up to 256 random patches with program changes in timed batches, resident or
    not — every buffer against the oracle.  Reaches the sites of the tests above in combinations they do not list."""
    from test_gpu_fuzz import random_patch
    rng = np.random.RandomState(int(os.environ.get("S2R_FUZZ_BASE", "1000")) * 29 + 13 + seed)
    max_frames = int(rng.choice(FUZZ_MAX_FRAMES))
    voices = int(rng.choice([8, 70, 300, 1000, 2100]))
    block = int(rng.choice([0, 64, 128, 256]))
    groups = int(rng.choice([0, 0, 2, 3]))
    n_bank = int(rng.choice([1, 1, 2, 5, 30, 256]))
    bank = [random_patch(rng) for _ in range(n_bank)]
    pr = Pair(voices, bank[0], max_frames=max_frames, block_voices=block, mix_groups=groups)
    if n_bank > 1:
        pr.set_bank(bank)
    pr.bank_size, pr.threads = n_bank, _threads()
    if voices * max_frames > 1 << 22:                     # (the oracle's share of a case stays at seconds)
        voices = 70
    resident = rng.rand() < 0.5
    if resident:
        pr.gpu.set_resident(True)
    what = "shape seed %d: %d voices, max_frames %d, block %d, groups %d, %d patches%s" % (
        seed, voices, max_frames, block, groups, n_bank, ", resident" if resident else "")
    ring = _Ring(pr, what)
    hist = None
    for b in range(8):
        form = str(rng.choice(["sample", "sample", "ring", "ring", "stereo", "voices", "oversampled"]))
        frames = int(rng.choice([1, 15, 16, 17, max_frames - 1, max_frames, max_frames, int(rng.randint(1, max_frames + 1))]))
        frames = min(max(1, frames), max_frames)
        ev = _events(rng, frames, int(rng.randint(0, 40)), n_bank, timed=form != "voices" and b > 0 and rng.rand() < 0.6,
                     first_on=voices if b == 0 else None)
        tag = "buffer %d (%s, %d frames)" % (b, form, frames)
        if form == "ring":
            ring.begin(ev, frames, tag)
            continue
        ring.drain()
        if form == "oversampled":
            n = max(1, frames // 4)
            if 4 * n > max_frames:
                continue
            ev = _events(rng, 4 * n, int(rng.randint(0, 10)), n_bank, timed=False)
            pr.gpu.note_events(ev)
            got = pr.gpu.sample_oversampled(n, SR)
            x = np.concatenate([hist if hist is not None else np.zeros(62, dtype=np.float32),
                                s2o.mix_tree(_oracle_rows(pr, ev, 4 * n, 4 * SR), pr.block_voices, pr.groups)])
            hist = x[-62:]
            assert_bits_equal(got, s2o.decimate4(x, n), "%s, %s" % (what, tag))
        else:
            _fill(pr, form, ev, frames, "%s, %s" % (what, tag))
    ring.drain()
    _assert_state_is_the_oracle_s(pr, what)
