"""The uniform window where tests/test_gpu_uniform_window.py never took it: windows of waves other than wave 0
and of several workgroups at once, runs that fill a whole plane, seeds other than 0 and offsets across 65 536, whole cohorts
released and restarted, the exit at 2^24, the forms that must have no window, and the entries other than sample and
render_voices with the switch on and off.

Every case compares bit for bit against the CPU oracle — per-voice rows where the case has no timed event, and the mix through
s2o.mix_tree — and against the same fills with the window switched off, and states the handle's counter of window chunks after
every fill as an exact list (all zeros with the switch off), derived in the case's docstring; the cases with timed events too.

48 kHz.  Note-ons take never-started voices in index order, so 64 consecutive note-ons are one wavefront; in a pool where every
voice is equally old they take the voices in index order too.  A wave goes through the window for a run of three chunks or more
during which both envelopes move (the amplitude flat: the flat-amplitude variant; the mod envelope flat: the cached constants),
every lane is started and shares offset, seed and stages, the offsets are multiples of 16 below 2^24, and the patch has no noise
level.  ENV turns: amp attack to frame 960, decay to 2400, release 1200 frames; mod attack to 480, decay to 3360, release 2400
frames.  LONG: both attacks to frame 4800, both decays to 9600."""
import numpy as np
import pytest

from helpers import assert_bits_equal, make_patch, oracle_cfg_from_patch
from oracle import s2o
import synth2_amd as s2
from test_gpu_uniform_window import ENV, NOTES, _events, _oracle

pytestmark = pytest.mark.gpu

SR = 48000
LONG = dict(ENV)
LONG.update({"amp_env.attack_ms": 100.0, "amp_env.decay_ms": 100.0, "mod_env.attack_ms": 100.0, "mod_env.decay_ms": 100.0})
SEED_LAST = 0x87ffffff                       # rotl(seed, 5) = 0xfffffff0: at offset 0 a chunk reads the noise table's last 16 entries


def _frames_of(ms, sr=SR):
    """Ms::as_samples (units.rs:44-53) in f32, as the host and the oracle evaluate it"""
    return float(np.float32(sr) * (np.float32(ms) / np.float32(1000.0)))


def _rotl5(seed):
    return ((seed << 5) | (seed >> 27)) & 0xffffffff


def test_the_turns_this_file_counts_with_are_whole_frames():
    """the docstrings' arithmetic rests on these: every envelope time used here is a whole number of 16-frame chunks"""
    for ms, frames in ((10.0, 480), (20.0, 960), (25.0, 1200), (30.0, 1440), (50.0, 2400), (60.0, 2880), (100.0, 4800), (1400.0, 67200)):
        assert _frames_of(ms) == frames and frames % 16 == 0, (ms, _frames_of(ms))
    for seed in (1024, SEED_LAST) + tuple((k + 1) << 10 for k in range(64)):
        assert _rotl5(seed) & 15 == 0, hex(seed)
    assert _rotl5(SEED_LAST) == 0xfffffff0


def _wave_on(k, n=64, frame=0):
    """the note-ons of wave k's first n lanes: every lane its own pitch, every wave its own rotation of NOTES"""
    return [(1, NOTES[(j + 7 * k) % 64], frame) for j in range(n)]


def _cohort_off(frame=0, lanes=range(64)):
    return [(0, NOTES[j], frame) for j in lanes]


def _oracle_aged(voices, patch, fills, events, sr, seeds, ages):
    """_oracle of tests/test_gpu_uniform_window.py with the ageing of `ages`: {fill: (voices, offset)} — before that fill's
    events the listed voices, started and not released, get current_frame_offset = offset (the GPU side gets the same edit)"""
    cpu = s2o.OracleSynth(voices)
    cpu.config = oracle_cfg_from_patch(patch)

    def apply(kind, note):
        if kind:
            v = cpu.next_voice_index()
            cpu.note_on(note)
            if seeds is not None:
                cpu.set_seed(v, int(seeds[v]))
        else:
            cpu.note_off(note)

    rows = []
    for b, frames in enumerate(fills):
        if b in ages:
            for v in ages[b][0]:
                vo = cpu.voice(int(v))
                assert vo.has_current and not vo.has_release
                vo.current_frame_offset = int(ages[b][1])
                vo.has_release = 0
                vo.release_frame_offset = 0
        ev = events.get(b, [])
        pv = np.zeros((voices, frames), dtype=np.float32)
        if not any(f for _k, _n, f in ev):
            for kind, note, _f in ev:
                apply(kind, note)
            pv[:, :] = cpu.render_voices(frames, sr)
        else:
            k = 0
            for c in range(0, frames, 16):
                while k < len(ev) and ev[k][2] == c:
                    apply(ev[k][0], ev[k][1])
                    k += 1
                n = min(16, frames - c)
                pv[:, c:c + n] = cpu.render_voices(n, sr)
            assert k == len(ev)
        rows.append(pv)
    return rows


def _gpu(voices, patch, fills, events, window, rows, seeds=None, block_voices=0, ages=None, sr=SR):
    """one GPU handle through the case: its outputs per fill (per-voice rows, or the mix), the counter after every fill, and the
    handle's workgroup size"""
    g = s2.Synth(voices, max_frames=1024, block_voices=block_voices)
    try:
        g.set_patch(patch)
        if seeds is not None:
            for v, sd in enumerate(seeds):
                if sd:
                    g.set_noise_seed(v, int(sd))
        if not window:
            g.set_uniform_window(False)
        outs, counts = [], []
        for b, frames in enumerate(fills):
            if ages and b in ages:
                st = g.export_state()
                for v in ages[b][0]:
                    assert st["started"][v] and not st["released"][v]
                    st["current_frame_offset"][v] = ages[b][1]
                    st["released"][v] = 0
                    st["release_frame_offset"][v] = 0
                g.import_state(st)
            if events.get(b):
                g.note_events(_events(events[b]))
            outs.append(g.render_voices(frames, sr) if rows else g.sample(np.empty(frames, dtype=np.float32), sr).copy())
            counts.append(g.uniform_window_chunks())
        return outs, counts, g.block_voices
    finally:
        g.close()


def _case(patch, fills, events, voices=256, seeds=None, block_voices=0, ages=None, finite=False):
    """Runs the case on the oracle once and on the GPU with the window on (the mix, and the rows where the case has no timed
    event) and off (the mix); asserts the bits and that the switched-off handle counts nothing; returns the window-on mix run's
    counter after every fill."""
    if ages:
        want = _oracle_aged(voices, patch, fills, events, SR, seeds, ages)
    else:
        want = _oracle(voices, patch, fills, events, SR, seeds)
    if finite:
        for b, w in enumerate(want):
            assert np.all(np.isfinite(w)), "the oracle is not finite in fill %d" % b
    timed = any(f for evs in events.values() for _k, _n, f in evs)
    mix_on, counts, bv = _gpu(voices, patch, fills, events, True, False, seeds, block_voices, ages)
    print("window chunks after every fill:", counts)
    mix_off, counts_off, _ = _gpu(voices, patch, fills, events, False, False, seeds, block_voices, ages)
    assert counts_off == [0] * len(fills), counts_off
    for b in range(len(fills)):
        assert_bits_equal(mix_on[b], s2o.mix_tree(want[b], bv, 1), "mix against the oracle, fill %d" % b)
        assert_bits_equal(mix_on[b], mix_off[b], "window on against off, fill %d" % b)
    if not timed:
        rows_on, counts_rows, _ = _gpu(voices, patch, fills, events, True, True, seeds, block_voices, ages)
        for b in range(len(fills)):
            assert_bits_equal(rows_on[b], want[b], "per-voice rows against the oracle, fill %d" % b)
        assert counts_rows == counts, (counts_rows, counts)
    return counts


# ---- 1. a full-length window ----

@pytest.mark.parametrize("osc", [s2.OSC_SAW, s2.OSC_SINE])
def test_runs_of_64_chunks_fill_every_plane_to_its_end(osc):
    """LONG, one cohort, five fills of 1024.  No envelope turns before frame 4800, so each of the first four fills is ONE run of 64
    chunks: uw_fill makes four passes of its q0 loop and writes all 1024 floats of each of the four planes, and the last chunk
    reads each plane's last 16.  The fifth fill (offsets 4096 .. 5120) is 44 chunks to the turn at 4800 and then 20."""
    counts = _case(make_patch(osc_kind=osc, **LONG), [1024] * 5, {0: _wave_on(0)})
    assert counts == [64, 128, 192, 256, 320], counts


# ---- 2. four waves, four windows ----

def test_four_windows_live_in_one_workgroup():
    """256 voices, fills of 256 frames (16 chunks), LONG; wave k's 64 note-ons come before fill k, k = 0 .. 3, and four more fills
    follow.  Every started wave is a cohort and runs its 16 chunks through its own window: fill k adds 16 * (min(k, 3) + 1).  From
    fill 3 on the four windows are live together with four different offsets (and so four different amplitude and coefficient
    lines), 768 frames apart at the most."""
    counts = _case(make_patch(**LONG), [256] * 8, {k: _wave_on(k) for k in range(4)})
    assert counts == [16, 48, 96, 160, 224, 288, 352, 416], counts


def test_four_windows_started_by_timed_note_ons():
    """In the first fill of 1024: wave 0 at frame 0, wave 1 at frame 160, wave 2 at frame 512; wave 3 at frame 0 of the second.
    The mix only.  Wave 0 renders the first fill's 64 chunks through its window.  A wave that waits for its start is not live: the
    run logic gives it one run that ends at its next event's frame (pick_run's `ne`), so the dense-event loop, which is entered
    two chunks or fewer ahead of an event, never is; the 64 restarts are applied at that boundary, no event is left, and the
    wave is a cohort from its first chunk: 54 chunks from frame 160, 32 from frame 512, 150 in all.  The second and third fill
    have no timed event and no turn (LONG): four cohorts, 64 chunks each, with offsets 1024, 864, 512 and 0 at the second
    fill's start, all multiples of 16."""
    ev = {0: _wave_on(0) + _wave_on(1, frame=160) + _wave_on(2, frame=512), 1: _wave_on(3)}
    counts = _case(make_patch(**LONG), [1024] * 3, ev)
    assert counts == [150, 406, 662], counts


# ---- 3. workgroup shapes ----

# (voices, block_voices, note-ons before fill 0 / 1 / 2, cohort waves in fill 0 / 1 / 2)
SHAPES = {
    # four workgroups of one wave: each window is the only one behind its workgroup's single tile
    "256_in_workgroups_of_64": (256, 64, (64, 128, 64), (1, 3, 4)),
    # two workgroups of two waves; wave 1 is a fill younger than wave 0, wave 3 a fill younger than wave 2
    "256_in_workgroups_of_128": (256, 128, (64, 128, 64), (1, 3, 4)),
    # three workgroups of four waves: waves 0-1 / 2-6 / 7-11 start before fill 0 / 1 / 2, so workgroups 0 and 1 each hold two offsets
    "768": (768, 0, (128, 320, 320), (2, 7, 12)),
    # the second workgroup has one started wave and three whose voices are out of range
    "320": (320, 256, (128, 128, 64), (2, 4, 5)),
    # the last wave holds 44 voices: 20 lanes have no voice, it is never a cohort
    "300": (300, 256, (128, 128, 44), (2, 4, 4)),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_workgroup_shapes(shape):
    """LONG, three fills of 512 frames (32 chunks, no turn).  Note-ons take the voices in index order; SHAPES says how many come
    before each fill and how many waves are cohorts in it — every wave whose 64 voices were started by one batch; the 44-voice
    wave of the 300-voice handle never is, and its rows still match.  Each cohort wave adds 32 chunks per fill: the counter is
    32 times the running sum of the cohort waves."""
    voices, bv, ons, cohorts = SHAPES[shape]
    events, v = {}, 0
    for b, n in enumerate(ons):
        events[b] = [(1, NOTES[(u + 7 * (u // 64)) % 64], 0) for u in range(v, v + n)]
        v += n
    assert v == voices
    counts = _case(make_patch(**LONG), [512] * 3, events, voices=voices, block_voices=bv)
    assert counts == [32 * sum(cohorts[:b + 1]) for b in range(3)], counts


def test_twelve_windows_in_three_workgroups_started_by_timed_note_ons():
    """768 voices, three workgroups of four waves, LONG, three fills of 512: wave w starts in fill w // 4 at frame 64 * (w % 4), so
    every wave of a workgroup has an offset of its own.  The mix only.  A wave is a cohort from the chunk of its start (see the
    timed case of four windows): the four new waves of a fill add 32 + 28 + 24 + 20 = 104 chunks, every wave that was already
    running 32: 104, then 104 + 4 * 32, then 104 + 8 * 32."""
    events = {b: [e for w in range(4 * b, 4 * b + 4) for e in _wave_on(w, frame=64 * (w % 4))] for b in range(3)}
    counts = _case(make_patch(**LONG), [512] * 3, events, voices=768)
    assert counts == [104, 336, 696], counts


# ---- 4. seeded cohorts ----

def test_seeded_cohorts_read_their_own_noise():
    """256 voices started together, LONG, five fills of 1024.  Wave 0 has seed 0, wave 1 seed 1024 (rotated: 0x8000), wave 2 seed
    0x87ffffff (rotated: 0xfffffff0 — at offset 0 its first chunk reads the noise table's last 16 entries), each the same on
    all 64 lanes and with a zero low nibble after the rotation: three cohorts.  Wave 3 has a seed per lane, (lane + 1) << 10,
    aligned too: only the window's own comparison of the seeds turns it away.  Three times the counts of one full-length
    window."""
    seeds = np.zeros(256, dtype=np.uint32)
    seeds[64:128] = 1024
    seeds[128:192] = SEED_LAST
    seeds[192:256] = [(k + 1) << 10 for k in range(64)]
    for sd in seeds:
        assert _rotl5(int(sd)) & 15 == 0
    events = {0: [e for w in range(4) for e in _wave_on(w)]}
    counts = _case(make_patch(**LONG), [1024] * 5, events, seeds=seeds)
    assert counts == [3 * c for c in (64, 128, 192, 256, 320)], counts


# ---- 5. across 65 536 ----

@pytest.mark.parametrize("seed,offset", [(0, 65536 - 512), (SEED_LAST, 65536 - 512), (0, 65536 - 504)])
def test_a_run_across_offset_65536(seed, offset):
    """Both attacks 1400 ms = 67 200 frames (the tables hold them: 70 080 entries of attack and decay).  A cohort is started, fills
    16 frames (one chunk: below the threshold of three), is aged to the offset and fills 1024 twice.  From 65 536 - 512 the first
    run is 64 chunks and its chunk 32 starts at offset 65 536, where the noise table's index wraps — with seed 0x87ffffff
    from entry 0x01f0 down to 0x0000 and on to 0xfff0; the second run ends at 67 072, before the turn.  65 536 - 504 is no
    multiple of 16: the wave is not aligned and the window is refused."""
    env = dict(ENV)
    env.update({"amp_env.attack_ms": 1400.0, "mod_env.attack_ms": 1400.0})
    seeds = None
    if seed:
        seeds = np.zeros(256, dtype=np.uint32)
        seeds[:64] = seed
    counts = _case(make_patch(**env), [16, 1024, 1024], {0: _wave_on(0)}, seeds=seeds, ages={1: (range(64), offset)})
    assert counts == ([0, 64, 128] if offset % 16 == 0 else [0, 0, 0]), counts


# ---- 6. released cohorts ----

def test_cohort_released_in_sustain():
    """ENV.  Four fills of 1024 (64, 64 and 22 chunks up to the amplitude's sustain at 2400, as in the first file), note-offs of
    all 64 notes before fill 4: the release starts at offset 4096, the amplitude's runs to 5296 and the mod envelope's to 6496,
    both on the later-release region of the tables (ru - 4096 + offset).  Fill 4 is one run of 64 chunks; fill 5 (5120 .. 6144)
    is 11 chunks to the amplitude's end at 5296, after which the amplitude is flat; fill 6 nothing."""
    counts = _case(make_patch(**ENV), [1024] * 7, {0: _wave_on(0), 4: _cohort_off()})
    assert counts == [64, 128, 150, 150, 214, 225, 225], counts


def test_cohort_released_in_the_decay():
    """Note-offs before fill 1: the release offset 1024 is clamped to attack + decay, so the amplitude releases over 2400 .. 3600
    and the mod envelope over 3360 .. 5760, on the clamped-release region of the tables (rc - rc_t0 + offset).  Fills 0 and 1: 64
    chunks each.  Fill 2 (2048 .. 3072): 22 chunks to 2400 and 42 behind it — the amplitude goes from its decay straight into
    the release and keeps moving.  Fill 3 (3072 .. 4096): 18 chunks to the mod envelope's turn at 3360, 15 to the amplitude's end
    at 3600, then flat.  Fill 4 nothing."""
    counts = _case(make_patch(**ENV), [1024] * 5, {0: _wave_on(0), 1: _cohort_off()})
    assert counts == [64, 128, 192, 225, 225], counts


def test_cohort_released_by_timed_note_offs():
    """the 64 note-offs at frame 512 of fill 4 (offset 4608): booked ahead, they end the sustain there, and the wave comes back to
    the window for the other 32 chunks of fill 4 and, in fill 5 (5120 .. 6144), for the 43 chunks up to the end of the amplitude's
    release at 5808.  The mix only."""
    counts = _case(make_patch(**ENV), [1024] * 7, {0: _wave_on(0), 4: _cohort_off(frame=512)})
    assert counts == [64, 128, 150, 150, 182, 225, 225], counts


def test_half_a_cohort_released():
    """lanes 0 .. 31 released before fill 4, the others never: the lanes' amplitude lines differ from then on, no cohort, and the
    counter stays where the sustain left it"""
    counts = _case(make_patch(**ENV), [1024] * 7, {0: _wave_on(0), 4: _cohort_off(lanes=range(32))})
    assert counts == [64, 128, 150, 150, 150, 150, 150], counts


def test_cohort_released_with_no_release_time():
    """release_ms 0 on both envelopes: a released voice is at its end at once, the amplitude flat: no window chunk after the sustain"""
    env = dict(ENV)
    env.update({"amp_env.release_ms": 0.0, "mod_env.release_ms": 0.0})
    counts = _case(make_patch(**env), [1024] * 7, {0: _wave_on(0), 4: _cohort_off()})
    assert counts == [64, 128, 150, 150, 150, 150, 150], counts


@pytest.mark.parametrize("frame", [0, 256])
def test_released_cohort_restarted(frame):
    """A pool of 64 voices: the late release above, then 64 new note-ons in fill 7 — every voice is equally old, so they take the
    voices in index order and restart every lane.  Before fill 7 (frame 0): the wave is a cohort again, runs of 30, 30 and 4
    chunks between the turns at 480 and 960 and the fill's end, 64 in all, and 64 more in fill 8 (1024 .. 2048, no turn).  At
    frame 256 of fill 7: the ended voices' run stops at the event's frame, the restarts are applied there and the 48 chunks
    behind them (offsets 0 .. 768: 30 to the turn at 480 and 18) take the window; fill 8 (offsets 768 .. 1792, no event) is 12
    chunks to the turn at 960 and 52 behind it."""
    ev = {0: _wave_on(0), 4: _cohort_off(), 7: _wave_on(0, frame=frame)}
    counts = _case(make_patch(**ENV), [1024] * 9, ev, voices=64)
    assert counts[:7] == [64, 128, 150, 150, 214, 225, 225], counts
    assert counts[7:] == ([289, 353] if frame == 0 else [273, 337]), counts


# ---- 7. the edge at 2^24 ----

def test_window_up_to_offset_2_to_the_24_and_not_beyond():
    """ENV with both releases 100 ms (4800 frames).  Four fills take the cohort into sustain (150 chunks); it is aged to offset
    2^24 - 2048 (the oracle's voices too) and all 64 notes are released there.  Fill 4 (.. 2^24 - 1024): both envelopes release,
    one run of 64 chunks.  Fill 5's last frame is 2^24 - 1: no offset of the fill passes 2^24, it still takes the window.  Fill 6
    starts at 2^24, where the tables and the f32 offsets end: in-lane coefficients, no window."""
    env = dict(ENV)
    env.update({"amp_env.release_ms": 100.0, "mod_env.release_ms": 100.0})
    counts = _case(make_patch(**env), [1024] * 7, {0: _wave_on(0), 4: _cohort_off()}, ages={4: (range(64), (1 << 24) - 2048)}, finite=True)
    assert counts == [64, 128, 150, 150, 214, 278, 278], counts


# ---- 8. no window ----

def test_no_window_with_a_noise_level():
    """noise = 0.25: the cheaper noise arithmetic the window builds on needs a level of 0.0"""
    counts = _case(make_patch(noise=0.25, **ENV), [1024, 1024], {0: _wave_on(0)})
    assert counts == [0, 0], counts


@pytest.mark.parametrize("form", ["low_latency", "resident_one_workgroup", "resident_two_workgroups"])
def test_no_window_in_the_resident_forms(form):
    """set_low_latency, and set_resident on a handle of one workgroup (which is set_low_latency) and of two (the pool-resident
    kernel): their launchers set no window.  The one-workgroup kernel takes a fill with at most nine untimed events, so the
    cohort's 64 note-ons go with a launch: that first fill is 16 frames, one chunk, below the threshold of three.  The two fills
    of 1024 behind it (offsets 16 .. 2064, across the turns at 480 and 960) would count 128 chunks with a window; the resident
    kernel is asserted to have run them.  The pool-resident kernel takes the note-ons itself."""
    voices = 512 if form == "resident_two_workgroups" else 256
    fills = [16, 1024, 1024]
    patch = make_patch(**ENV)
    want = _oracle(voices, patch, fills, {0: _wave_on(0)}, SR, None)
    outs = {}
    for window in (True, False):
        g = s2.Synth(voices, max_frames=1024)
        try:
            g.set_patch(patch)
            g.set_uniform_window(window)
            if form == "low_latency":
                g.set_low_latency(True)
            else:
                g.set_resident(True)
            g.note_events(_events(_wave_on(0)))
            outs[window] = []
            for b, frames in enumerate(fills):
                outs[window].append(g.sample(np.empty(frames, dtype=np.float32), SR).copy())
                if b or voices == 512:
                    assert g.resident_active, "fill %d did not go to the resident kernel" % b
                assert g.uniform_window_chunks() == 0, "fill %d" % b
            bv = g.block_voices
        finally:
            g.close()
    for b in range(len(fills)):
        assert_bits_equal(outs[True][b], s2o.mix_tree(want[b], bv, 1), "mix against the oracle, fill %d" % b)
        assert_bits_equal(outs[True][b], outs[False][b], "window on against off, fill %d" % b)


# ---- 9. the other entries, switch on against switch off ----

def _entry_fill(g, entry, frames):
    """one fill through `entry`: a list of arrays, everything the entry returns"""
    if entry == "sample":
        return [g.sample(np.empty(frames, dtype=np.float32), SR).copy()]
    if entry == "begin_end":
        g.sample_begin(frames, SR)
        return [g.sample_end(np.empty(frames, dtype=np.float32)).copy()]
    if entry == "render_voices":
        return [g.render_voices(frames, SR)]
    if entry == "fill_device":
        import torch
        row = torch.zeros(frames, dtype=torch.float32, device="cuda")
        g.fill_device(row.data_ptr(), frames, SR, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [row.cpu().numpy()]
    if entry == "panned":
        return [g.sample_panned(frames, SR).copy()]
    if entry == "buses":
        return [g.sample_buses(frames, SR, n_buses=2).copy()]
    assert entry == "master"
    master, stems = g.sample_master(frames, SR, n_buses=2)
    return [master.copy(), stems.copy()]


def _entry_run(entry, window, voices, n_on, **kw):
    g = s2.Synth(voices, max_frames=1024, **kw)
    try:
        g.set_patch(make_patch(**ENV))
        g.set_uniform_window(window)
        g.note_events(_events([(1, NOTES[(u + 7 * (u // 64)) % 64], 0) for u in range(n_on)]))
        outs, counts = [], []
        for frames in (512, 512):
            outs.append(_entry_fill(g, entry, frames))
            counts.append(g.uniform_window_chunks())
        return outs, counts
    finally:
        g.close()


def _entry_case(entry, voices, n_on, **kw):
    on, counts = _entry_run(entry, True, voices, n_on, **kw)
    off, counts_off = _entry_run(entry, False, voices, n_on, **kw)
    assert counts_off == [0, 0], counts_off
    for b in range(2):
        assert len(on[b]) == len(off[b])
        for k in range(len(on[b])):
            assert_bits_equal(on[b][k], off[b][k], "%s, window on against off, fill %d, output %d" % (entry, b, k))
    return counts


@pytest.mark.parametrize("entry", ["sample", "begin_end", "fill_device", "panned", "buses", "master"])
def test_other_entries_with_the_switch_on_and_off(entry):
    """One cohort in a 256-voice handle, ENV, two fills of 512.  Through sample: 30 chunks to the turn at 480 and two more, too
    few; then 28 to the turn at 960 and four more: [30, 62].  Every entry here renders its voices with the launch-per-fill
    kernel of one 256-voice workgroup and whole-fill super-chunks, the form that has the window: sample_begin / sample_end and
    fill_device through the same enqueue_fill as sample; sample_panned, sample_buses and sample_master render per-voice rows in
    slices of up to max_frames frames (pan_segment) with that kernel before their own mixdown.  So each counts what sample
    counts."""
    counts = _entry_case(entry, 256, 64)
    assert counts == [30, 62], (entry, counts)


@pytest.mark.parametrize("entry", ["sample", "begin_end", "render_voices"])
def test_device_list_handle_with_the_switch_on_and_off(entry):
    """devices=[0, 0]: 256 voices in two shards of one 128-voice workgroup; 192 note-ons start both waves of shard 0 and the first
    of shard 1.  The switch reaches the shards through `kids`, and the counter is the shards' sum: three cohorts, [90, 186].  (The
    mixer entries and fill_device refuse a device-list handle.)"""
    counts = _entry_case(entry, 256, 192, block_voices=128, devices=[0, 0])
    assert counts == [90, 186], (entry, counts)
