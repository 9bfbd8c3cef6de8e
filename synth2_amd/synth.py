"""Host-side mirror of ``s2_lib::try3::synth`` over the C ABI of libs2r (include/s2r.h).

Python is only the test / bench driver here (the reference's host language, Rust, is not in
this image; rust/s2_lib_gpu holds the uncompiled Rust shim and include/s2_synth.hpp the C++
one).  Names and argument meaning follow the reference
(/root/reference/components/s2_lib/src/try3/synth.rs:9-21,53-80,154-156;
units.rs:11-14):

    synth = Synth()                      # Synth::new()
    synth.note_on(Note(69), Velocity(1.0))
    synth.sample(buffer, SampleRateKhz(48000))
    synth.note_off(Note(69))

There is no CPU fallback: importing works anywhere, constructing a Synth needs libs2r.so and
a gfx950 device and raises otherwise.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

OSC_SQUARE, OSC_SAW, OSC_TRIANGLE, OSC_SINE = 0, 1, 2, 3
OSC_DPW_SAW, OSC_DPW_SQUARE, OSC_DPW_TRIANGLE = 4, 5, 6      # build-defined alias-suppressed shapes

S2R_OK = 0
S2R_ERR_INVALID = -1
S2R_ERR_NO_DEVICE = -2
S2R_ERR_HIP = -3
S2R_ERR_PATCH_SYNTAX = -4
S2R_ERR_PATCH_RANGE = -5
S2R_ERR_TOO_MANY_FRAMES = -6
S2R_ERR_OFFSET_OVERFLOW = -7
S2R_ERR_OUT_OF_MEMORY = -8
MAX_BUSES = 8                               # S2R_MAX_BUSES
MAX_IR_TAPS = 65536                         # S2R_MAX_IR_TAPS
MAX_DELAY_FRAMES = 262144                   # S2R_MAX_DELAY_FRAMES
CHORUS_MAX_VOICES = 8                       # S2R_CHORUS_MAX_VOICES
CHORUS_MAX_DELAY = 4095.0                   # S2R_CHORUS_MAX_DELAY
EQ_MAX_BANDS = 4                            # S2R_EQ_MAX_BANDS
EQ_PEAK, EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_LOWPASS, EQ_HIGHPASS = range(5)     # s2r_eq_kind
DYN_CURVE_POINTS = 513                      # S2R_DYN_CURVE_POINTS
ROOM_COMBS = 8                              # S2R_ROOM_COMBS
ROOM_ALLPASSES = 4                          # S2R_ROOM_ALLPASSES
ROOM_MIN_DELAY = 64                         # S2R_ROOM_MIN_DELAY
ROOM_MAX_DELAY = 8192                       # S2R_ROOM_MAX_DELAY
DRIVE_OVERSAMPLE = 4                        # S2R_DRIVE_OVERSAMPLE
DRIVE_TAPS = 65                             # S2R_DRIVE_TAPS
DRIVE_LATENCY = 16                          # S2R_DRIVE_LATENCY
DRIVE_HISTORY = 32                          # S2R_DRIVE_HISTORY
DRIVE_CURVE_POINTS = 1025                   # S2R_DRIVE_CURVE_POINTS
DRIVE_MAX_PRE = 1024.0                      # S2R_DRIVE_MAX_PRE
DRIVE_LINEAR, DRIVE_TANH, DRIVE_HARD, DRIVE_CUBIC, DRIVE_FOLD = range(5)     # s2r_drive_kind
FLANGER_MIN_DELAY = 32.0                    # S2R_FLANGER_MIN_DELAY
FLANGER_MAX_DELAY = 4095.0                  # S2R_FLANGER_MAX_DELAY
IR_SEGMENT = 256                            # S2R_IR_SEGMENT
METER_BLOCK = 256                           # S2R_METER_BLOCK
LIMITER_MAX_LOOKAHEAD = 1024                # S2R_LIMITER_MAX_LOOKAHEAD
LIMITER_MAX_HOLD = 4096                     # S2R_LIMITER_MAX_HOLD
LIMITER_CEILING_LOG2 = 20                   # S2R_LIMITER_CEILING_LOG2
LIMITER_SAMPLE_PEAK = 0                     # S2R_LIMITER_SAMPLE_PEAK
LIMITER_TRUE_PEAK = 1                       # S2R_LIMITER_TRUE_PEAK
LIMITER_TP_LATENCY = 8                      # S2R_LIMITER_TP_LATENCY
LIMITER_TP_HISTORY = 16                     # S2R_LIMITER_TP_HISTORY
LOUDNESS_PROGRAMMES = 9                     # S2R_LOUDNESS_PROGRAMMES: the buses, then the master
LOUDNESS_CHANNELS = 18                      # S2R_LOUDNESS_CHANNELS
LOUDNESS_STATE = 122                        # S2R_LOUDNESS_STATE
LOUDNESS_MIN_HOP, LOUDNESS_MAX_HOP = 16, 1 << 20      # S2R_LOUDNESS_MIN_HOP, S2R_LOUDNESS_MAX_HOP
LOUDNESS_MIN_HOPS, LOUDNESS_MAX_HOPS = 30, 1 << 18    # S2R_LOUDNESS_MIN_HOPS, S2R_LOUDNESS_MAX_HOPS
SPECTRUM_PROGRAMMES = 9                     # S2R_SPECTRUM_PROGRAMMES: the buses, then the master
SPECTRUM_MIN_FFT, SPECTRUM_MAX_FFT = 256, 8192        # S2R_SPECTRUM_MIN_FFT, S2R_SPECTRUM_MAX_FFT
SPECTRUM_MIN_HOP, SPECTRUM_MAX_HOP = 16, 1 << 20      # S2R_SPECTRUM_MIN_HOP, S2R_SPECTRUM_MAX_HOP (and at least n_fft / 8)
SPECTRUM_MAX_ROWS = 256                     # S2R_SPECTRUM_MAX_ROWS
WINDOW_RECT, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN_HARRIS = 0, 1, 2, 3      # S2R_WINDOW_*
PCM_PROGRAMMES, PCM_CHANNELS, PCM_MAX_TAPS, PCM_STATE = 9, 18, 9, 162         # S2R_PCM_PROGRAMMES, S2R_PCM_CHANNELS, S2R_PCM_MAX_TAPS, S2R_PCM_STATE
PCM_MIN_BITS, PCM_MAX_BITS, PCM_MAX_TAP = 8, 24, 16.0                    # S2R_PCM_MIN_BITS, S2R_PCM_MAX_BITS, S2R_PCM_MAX_TAP
DITHER_NONE, DITHER_RECT, DITHER_TRI = 0, 1, 2                           # S2R_DITHER_*
SHAPER_FLAT, SHAPER_FIRST, SHAPER_SECOND, SHAPER_3TAP, SHAPER_5TAP, SHAPER_9TAP = 0, 1, 2, 3, 4, 5       # S2R_SHAPER_*
RESAMPLER_PROGRAMMES, RESAMPLER_CHANNELS = 9, 18                         # S2R_RESAMPLER_PROGRAMMES, S2R_RESAMPLER_CHANNELS
RESAMPLER_MAX_FACTOR, RESAMPLER_MIN_TAPS, RESAMPLER_MAX_TAPS = 320, 4, 128         # S2R_RESAMPLER_MAX_FACTOR, S2R_RESAMPLER_MIN_TAPS, S2R_RESAMPLER_MAX_TAPS
RESAMPLER_MAX_TABLE, RESAMPLER_MAX_TAP = 24576, 4.0                      # S2R_RESAMPLER_MAX_TABLE, S2R_RESAMPLER_MAX_TAP
RESAMPLER_MAX_RATIO = 4                                          # s2r.h, s2r_set_master_resampler: L / M within 1/4 .. 4
_DITHER_KINDS = {"none": DITHER_NONE, "rect": DITHER_RECT, "rpdf": DITHER_RECT, "rectangular": DITHER_RECT, "tri": DITHER_TRI, "tpdf": DITHER_TRI,
                 "triangular": DITHER_TRI}
_WINDOW_KINDS = {"rect": WINDOW_RECT, "rectangular": WINDOW_RECT, "hann": WINDOW_HANN, "hamming": WINDOW_HAMMING,
                 "blackman-harris": WINDOW_BLACKMAN_HARRIS, "blackmanharris": WINDOW_BLACKMAN_HARRIS}


class S2rError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libs2r status %d: %s" % (status, message))
        self.status = status


class Adsr(C.Structure):
    """static_config.rs:38-44"""
    _fields_ = [("attack_ms", C.c_float), ("decay_ms", C.c_float), ("sustain", C.c_float), ("release_ms", C.c_float)]


class Patch(C.Structure):
    """static_config.rs:4-24 (sc::Layer)"""
    _fields_ = [("osc_kind", C.c_int32), ("osc_gain", C.c_float), ("noise", C.c_float), ("lpf_freq", C.c_float),
                ("amp_env", Adsr), ("mod_env", Adsr),
                ("mod_env_to_osc_freq", C.c_float), ("mod_env_to_lpf_freq", C.c_float),
                ("lpf_kind", C.c_int32), ("lpf_damping", C.c_float), ("lpf_q", C.c_float)]


# s2r_filter_kind: filters.rs one-pole (the reference's live path) and dsp_filters.rs:25-180
FILT_ONEPOLE, FILT_LP1, FILT_HP1, FILT_LP2, FILT_HP2, FILT_BP2 = 0, 1, 2, 3, 4, 5
FILT_SVF_LP, FILT_SVF_BP, FILT_SVF_HP = 6, 7, 8      # build-defined state-variable filter


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("total_voices", C.c_uint32), ("shard_begin", C.c_uint32),
                ("shard_voices", C.c_uint32), ("max_frames", C.c_uint32), ("device", C.c_int32),
                ("block_voices", C.c_uint32), ("mix_groups", C.c_uint32), ("reserved0", C.c_uint32),
                ("shard_interleave", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("n_devices", C.c_uint32), ("devices", C.c_int32 * 16)]


class VoiceState(C.Structure):
    _fields_ = [("note", C.c_uint8), ("started", C.c_uint8), ("released", C.c_uint8), ("program", C.c_uint8),
                ("current_frame_offset", C.c_uint32), ("release_frame_offset", C.c_uint32),
                ("pitch_hz", C.c_float), ("phase_accum", C.c_float), ("lpf_last", C.c_float),
                ("noise_seed", C.c_uint32), ("velocity", C.c_float),
                ("filt_x1", C.c_float), ("filt_x2", C.c_float), ("filt_y1", C.c_float), ("filt_y2", C.c_float),
                ("osc_z", C.c_float)]


VOICE_STATE_DTYPE = np.dtype([("note", np.uint8), ("started", np.uint8), ("released", np.uint8), ("program", np.uint8),
                              ("current_frame_offset", np.uint32), ("release_frame_offset", np.uint32),
                              ("pitch_hz", np.float32), ("phase_accum", np.float32), ("lpf_last", np.float32),
                              ("noise_seed", np.uint32), ("velocity", np.float32),
                              ("filt_x1", np.float32), ("filt_x2", np.float32), ("filt_y1", np.float32), ("filt_y2", np.float32),
                              ("osc_z", np.float32)])
assert VOICE_STATE_DTYPE.itemsize == C.sizeof(VoiceState)
LAYER_CALL_DTYPE = np.dtype([("pitch_hz", np.float32), ("offset", np.uint32), ("release_offset", np.uint32),
                             ("has_release", np.uint8), ("program", np.uint8), ("_pad", np.uint8, (2,)),
                             ("phase_accum", np.float32), ("lpf_last", np.float32), ("noise_seed", np.uint32),
                             ("filt_x1", np.float32), ("filt_x2", np.float32), ("filt_y1", np.float32), ("filt_y2", np.float32),
                             ("osc_z", np.float32)])
assert LAYER_CALL_DTYPE.itemsize == 48
VOICE_LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint8)
NOTE_EVENT_DTYPE = np.dtype([("kind", np.uint8), ("note", np.uint8), ("frame", np.uint16), ("velocity", np.float32)])
assert NOTE_EVENT_DTYPE.itemsize == 8


class Note(int):
    """synth.rs:16 ``pub struct Note(pub u8)``"""
    def __new__(cls, v):
        if not 0 <= int(v) <= 255:
            raise ValueError("Note is a u8")
        return super().__new__(cls, int(v))


class Velocity(float):
    """synth.rs:18 ``pub struct Velocity(pub Unipolar<1>)`` (stored, never used in rendering)"""


class SampleRateKhz(int):
    """units.rs:14 — named Khz in the reference but holds Hz (units.rs:21)"""


_lib = None
_f32p = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)


def lib_path():
    return _build.LIB


def load_library():
    """dlopen libs2r.so; builds it first when it was not built from the sources on disk (s2r_build_id: content, not times)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if _build.needs_build():
        # no library, or one built from other sources: rebuild, and fail loudly if that is impossible — a stale
        # libs2r.so would let tests and the bench pass against old code
        try:
            path = _build.build()
        except Exception as e:
            raise RuntimeError("libs2r.so is missing or was not built from these sources (build id %s, sources %s) and could not be rebuilt: %s" % (
                _build.embedded_build_id(), _build.build_id(), e)) from e
    L = C.CDLL(path)
    if not _build.AB_LIB:
        L.s2r_build_id.restype = C.c_char_p
        have = L.s2r_build_id().decode()
        if have != _build.build_id():
            raise RuntimeError("libs2r.so says it was built from %s; the sources on disk are %s" % (have, _build.build_id()))
    H = C.c_void_p
    sig = {
        "s2r_abi_version": (C.c_uint32, []),
        "s2r_build_id": (C.c_char_p, []),
        "s2r_status_string": (C.c_char_p, [C.c_int]),
        "s2r_create": (C.c_int, [C.POINTER(Config), C.POINTER(H)]),
        "s2r_destroy": (None, [H]),
        "s2r_load_patch": (C.c_int, [H, C.c_char_p, C.c_size_t]),
        "s2r_set_patch": (C.c_int, [H, C.POINTER(Patch)]),
        "s2r_get_patch": (C.c_int, [H, C.POINTER(Patch)]),
        "s2r_stream_frame_json": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]),
        "s2r_set_patch_bank": (C.c_int, [H, C.POINTER(Patch), C.c_uint32]),
        "s2r_patch_bank_size": (C.c_uint32, [H]),
        "s2r_program_change": (C.c_int, [H, C.c_uint32]),
        "s2r_default_patch": (None, [C.POINTER(Patch)]),
        "s2r_note_on": (C.c_int, [H, C.c_uint8, C.c_float]),
        "s2r_note_on_ex": (C.c_int, [H, C.c_uint8, C.c_float, C.POINTER(C.c_uint32)]),
        "s2r_note_off": (C.c_int, [H, C.c_uint8]),
        "s2r_note_events": (C.c_int, [H, C.c_void_p, C.c_size_t]),
        "s2r_fill": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_fill_begin": (C.c_int, [H, C.c_size_t, C.c_uint32]),
        "s2r_fill_end": (C.c_int, [H, _f32p, C.c_size_t]),
        "s2r_fill_pending_frames": (C.c_size_t, [H]),
        "s2r_fills_in_flight": (C.c_uint32, [H]),
        "s2r_fill_stereo": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_fill_oversampled": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_set_program_pan": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float]),
        "s2r_get_program_pan": (C.c_int, [H, C.c_uint32, _f32p, _f32p]),
        "s2r_get_voice_pans": (C.c_int, [H, _f32p]),
        "s2r_set_voice_pans": (C.c_int, [H, _f32p]),
        "s2r_fill_panned": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_voice_pan": (C.c_float, [C.c_float, C.c_float, C.c_uint8]),
        "s2r_pan_gains": (None, [C.c_float, _f32p, _f32p]),
        "s2r_set_program_mix": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float, C.c_uint32]),
        "s2r_get_program_mix": (C.c_int, [H, C.c_uint32, _f32p, _f32p, C.POINTER(C.c_uint32)]),
        "s2r_get_voice_mix": (C.c_int, [H, _f32p, C.POINTER(C.c_uint8)]),
        "s2r_set_voice_mix": (C.c_int, [H, _f32p, C.POINTER(C.c_uint8)]),
        "s2r_voice_gain": (C.c_float, [C.c_float, C.c_float, C.c_float]),
        "s2r_fill_buses": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32]),
        "s2r_set_program_fader": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float]),
        "s2r_get_program_fader": (C.c_int, [H, C.c_uint32, _f32p, _f32p, _f32p, _f32p]),
        "s2r_snap_program_faders": (C.c_int, [H]),
        "s2r_fader_gains": (None, [C.c_float, C.c_float, C.c_float, C.c_float, _f32p, _f32p]),
        "s2r_set_program_send": (C.c_int, [H, C.c_uint32, C.c_float, C.c_uint32]),
        "s2r_get_program_send": (C.c_int, [H, C.c_uint32, _f32p, C.POINTER(C.c_uint32)]),
        "s2r_get_voice_sends": (C.c_int, [H, _f32p, C.POINTER(C.c_uint8)]),
        "s2r_set_voice_sends": (C.c_int, [H, _f32p, C.POINTER(C.c_uint8)]),
        "s2r_send_gain": (C.c_float, [C.c_float, C.c_float]),
        "s2r_set_bus_reverb": (C.c_int, [H, C.c_uint32, _f32p, _f32p, C.c_uint32, C.c_float, C.c_float]),
        "s2r_set_bus_reverb_mix": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float]),
        "s2r_get_bus_reverb": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint32), _f32p, _f32p]),
        "s2r_get_bus_reverb_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_reverb_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_reverb_reference": (C.c_int, [_f32p, C.c_uint32, _f32p, C.c_uint32, C.c_float, C.c_float, _f32p]),
        "s2r_set_bus_delay": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float]),
        "s2r_set_bus_delay_mix": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float]),
        "s2r_get_bus_delay": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint32), _f32p, _f32p, _f32p, _f32p]),
        "s2r_get_bus_delay_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_delay_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_delay_reference": (C.c_int, [C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, _f32p, C.c_uint32, _f32p, _f32p]),
        "s2r_chorus_history_frames": (C.c_uint32, [C.c_float, C.c_float]),
        "s2r_set_bus_chorus": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float]),
        "s2r_set_bus_chorus_mix": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float]),
        "s2r_set_bus_chorus_rate": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_uint32]),
        "s2r_get_bus_chorus": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint32), _f32p, _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _f32p, _f32p]),
        "s2r_get_bus_chorus_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_bus_chorus_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_chorus_reference": (C.c_int, [C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float, _f32p, C.c_uint32, _f32p,
                                           C.POINTER(C.c_uint32), _f32p]),
        "s2r_set_bus_eq": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p]),
        "s2r_set_bus_eq_coeffs": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p]),
        "s2r_get_bus_eq": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint32), _f32p, C.c_size_t]),
        "s2r_get_bus_eq_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_eq_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_eq_reference": (C.c_int, [C.c_uint32, _f32p, _f32p, C.c_uint32, _f32p, _f32p]),
        "s2r_eq_design": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, _f32p]),
        "s2r_set_bus_dynamics": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p, C.c_float, C.c_float]),
        "s2r_clear_bus_dynamics": (C.c_int, [H, C.c_uint32]),
        "s2r_set_bus_dynamics_params": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p, C.c_float, C.c_float]),
        "s2r_get_bus_dynamics": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _f32p, C.c_size_t, _f32p, _f32p]),
        "s2r_get_bus_dynamics_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_dynamics_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_get_bus_dynamics_meter": (C.c_int, [H, C.c_uint32, _f32p]),
        "s2r_dynamics_reference": (C.c_int, [_f32p, C.c_float, C.c_float, _f32p, _f32p, C.c_uint32, _f32p, _f32p, _f32p]),
        "s2r_dynamics_curve": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, _f32p]),
        "s2r_dynamics_coef": (C.c_float, [C.c_double, C.c_double]),
        "s2r_set_bus_room": (C.c_int, [H, C.c_uint32, _u32p, _u32p, C.c_uint32] + [C.c_float] * 7),
        "s2r_clear_bus_room": (C.c_int, [H, C.c_uint32]),
        "s2r_set_bus_room_params": (C.c_int, [H, C.c_uint32] + [C.c_float] * 7),
        "s2r_get_bus_room": (C.c_int, [H, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _f32p]),
        "s2r_get_bus_room_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_room_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_room_state_floats": (C.c_size_t, [_u32p, _u32p, C.c_uint32]),
        "s2r_room_reference": (C.c_int, [_u32p, _u32p, C.c_uint32] + [C.c_float] * 7 + [_f32p, C.c_uint32, _f32p, _f32p]),
        "s2r_room_design": (C.c_int, [C.c_double, C.c_double, _u32p, _u32p, _u32p]),
        "s2r_set_bus_drive": (C.c_int, [H, C.c_uint32, _f32p, C.c_float, C.c_float, C.c_float]),
        "s2r_clear_bus_drive": (C.c_int, [H, C.c_uint32]),
        "s2r_set_bus_drive_params": (C.c_int, [H, C.c_uint32, _f32p, C.c_float, C.c_float, C.c_float]),
        "s2r_get_bus_drive": (C.c_int, [H, C.c_uint32, _u32p, _f32p, C.c_size_t, _f32p, _f32p, _f32p]),
        "s2r_get_bus_drive_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_set_bus_drive_history": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t]),
        "s2r_drive_reference": (C.c_int, [_f32p, C.c_float, C.c_float, C.c_float, _f32p, C.c_uint32, _f32p, _f32p]),
        "s2r_drive_taps": (C.c_int, [_f32p]),
        "s2r_drive_curve": (C.c_int, [C.c_uint32, C.c_double, _f32p]),
        "s2r_flanger_history_frames": (C.c_uint32, [C.c_float, C.c_float]),
        "s2r_set_bus_flanger": (C.c_int, [H, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float]),
        "s2r_clear_bus_flanger": (C.c_int, [H, C.c_uint32]),
        "s2r_set_bus_flanger_params": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float]),
        "s2r_get_bus_flanger": (C.c_int, [H, C.c_uint32, _f32p, _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _f32p, _f32p, _f32p, _f32p]),
        "s2r_get_bus_flanger_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_bus_flanger_state": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_flanger_reference": (C.c_int, [C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, _f32p, C.c_uint32, _f32p,
                                            C.POINTER(C.c_uint32), _f32p]),
        "s2r_set_bus_return": (C.c_int, [H, C.c_uint32, C.c_float]),
        "s2r_get_bus_return": (C.c_int, [H, C.c_uint32, _f32p, _f32p]),
        "s2r_set_master_fader": (C.c_int, [H, C.c_float]),
        "s2r_get_master_fader": (C.c_int, [H, _f32p, _f32p]),
        "s2r_snap_master": (C.c_int, [H]),
        "s2r_fill_master": (C.c_int, [H, _f32p, _f32p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32]),
        "s2r_get_meters": (C.c_int, [H, C.POINTER(C.c_uint32), _f32p, _f32p, C.c_size_t]),
        "s2r_master_reference": (C.c_int, [_f32p, C.c_uint32, C.c_uint32, _f32p, _f32p, C.c_float, C.c_float, _f32p, _f32p, _f32p]),
        "s2r_set_master_limiter": (C.c_int, [H, C.c_float, C.c_uint32, C.c_uint32]),
        "s2r_clear_master_limiter": (C.c_int, [H]),
        "s2r_get_master_limiter": (C.c_int, [H, _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "s2r_get_limiter_state": (C.c_int, [H, _f32p, C.c_size_t, _f32p, C.c_size_t]),
        "s2r_set_limiter_state": (C.c_int, [H, _f32p, C.c_size_t, _f32p, C.c_size_t]),
        "s2r_get_limiter_meters": (C.c_int, [H, _f32p, _f32p]),
        "s2r_limiter_reference": (C.c_int, [_f32p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, _f32p]),
        "s2r_set_master_limiter_ex": (C.c_int, [H, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32]),
        "s2r_get_master_limiter_detector": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "s2r_limiter_tp_reference": (C.c_int, [_f32p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, _f32p]),
        "s2r_set_master_loudness": (C.c_int, [H, _f32p, C.c_uint32, C.c_uint32]),
        "s2r_clear_master_loudness": (C.c_int, [H]),
        "s2r_get_master_loudness": (C.c_int, [H, _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
        "s2r_reset_master_loudness": (C.c_int, [H]),
        "s2r_get_loudness": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_double)]),
        "s2r_get_true_peak": (C.c_int, [H, _f32p, _f32p]),
        "s2r_get_loudness_state": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_loudness_state": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_get_loudness_hops": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_set_loudness_hops": (C.c_int, [H, _f32p, C.c_size_t, C.c_size_t]),
        "s2r_loudness_reference": (C.c_int, [_f32p, C.c_uint32, _f32p, C.c_uint32, _f32p, C.c_uint32, _f32p, C.POINTER(C.c_uint32), _f32p, C.c_size_t,
                                             C.POINTER(C.c_size_t), _f32p]),
        "s2r_loudness_readings": (C.c_int, [_f32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
        "s2r_loudness_design": (C.c_int, [C.c_double, _f32p]),
        "s2r_set_master_spectrum": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p, C.c_uint32]),
        "s2r_clear_master_spectrum": (C.c_int, [H]),
        "s2r_get_master_spectrum": (C.c_int, [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), _f32p, C.c_size_t]),
        "s2r_reset_master_spectrum": (C.c_int, [H]),
        "s2r_get_spectrum": (C.c_int, [H, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_size_t]),
        "s2r_get_spectrum_bands": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
        "s2r_get_spectrum_rows": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_set_spectrum_rows": (C.c_int, [H, _f32p, C.c_size_t, C.c_size_t]),
        "s2r_get_spectrum_state": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_spectrum_state": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_spectrum_reference": (C.c_int, [C.c_uint32, C.c_uint32, _f32p, _f32p, C.c_uint32, _f32p, C.c_uint32, _f32p, C.POINTER(C.c_uint32), _f32p, C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
        "s2r_spectrum_readings": (C.c_int, [_f32p, C.c_size_t, C.c_uint32, _f32p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_size_t]),
        "s2r_spectrum_band_readings": (C.c_int, [_f32p, C.c_size_t, C.c_uint32, _f32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_spectrum_window": (C.c_int, [C.c_uint32, C.c_uint32, _f32p]),
        "s2r_spectrum_twiddles": (C.c_int, [C.c_uint32, _f32p]),
        "s2r_set_master_pcm": (C.c_int, [H, C.c_uint32, C.c_uint32, _f32p, C.c_uint32, C.c_uint32]),
        "s2r_clear_master_pcm": (C.c_int, [H]),
        "s2r_get_master_pcm": (C.c_int, [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "s2r_reset_master_pcm": (C.c_int, [H]),
        "s2r_get_pcm": (C.c_int, [H, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_get_pcm_clips": (C.c_int, [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "s2r_get_pcm_state": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_pcm_state": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_pcm_reference": (C.c_int, [C.c_uint32, C.c_uint32, _f32p, C.c_uint32, C.c_uint32, _f32p, C.c_uint32, _f32p, C.c_uint32, _f32p, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
        "s2r_pcm_dither": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
        "s2r_pcm_pack": (C.c_int, [C.POINTER(C.c_int32), C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]),
        "s2r_pcm_shaper": (C.c_int, [C.c_uint32, _f32p, C.POINTER(C.c_uint32)]),
        "s2r_set_master_resampler": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_uint32, _f32p]),
        "s2r_clear_master_resampler": (C.c_int, [H]),
        "s2r_get_master_resampler": (C.c_int, [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _f32p]),
        "s2r_reset_master_resampler": (C.c_int, [H]),
        "s2r_get_resampled": (C.c_int, [H, C.c_uint32, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_get_resampler_state": (C.c_int, [H, _f32p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "s2r_set_resampler_state": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_resampler_reference": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, C.c_uint32, _f32p, C.c_uint32, _f32p, C.POINTER(C.c_uint32), _f32p,
                                              C.c_size_t, C.POINTER(C.c_size_t)]),
        "s2r_resampler_count": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]),
        "s2r_resampler_design": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, _f32p]),
        "s2r_set_master_multiband": (C.c_int, [H, C.c_uint32, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
        "s2r_set_master_multiband_params": (C.c_int, [H, C.c_uint32, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
        "s2r_clear_master_multiband": (C.c_int, [H]),
        "s2r_get_master_multiband": (C.c_int, [H, C.POINTER(C.c_uint32), _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
        "s2r_reset_master_multiband": (C.c_int, [H]),
        "s2r_get_multiband_state": (C.c_int, [H, _f32p, C.c_size_t]),
        "s2r_set_multiband_state": (C.c_int, [H, _f32p, C.c_size_t]),
        "s2r_get_multiband_meters": (C.c_int, [H, _f32p, C.c_size_t]),
        "s2r_multiband_reference": (C.c_int, [C.c_uint32, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_uint32, _f32p, _f32p, _f32p, _f32p]),
        "s2r_multiband_design": (C.c_int, [C.c_double, C.POINTER(C.c_double), C.c_uint32, _f32p, _f32p, _f32p]),
        "s2r_fill_device": (C.c_int, [H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
        "s2r_fill_device_root": (C.c_int, [H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
        "s2r_sum_partials_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]),
        "s2r_render_voices": (C.c_int, [H, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_process_layers": (C.c_int, [H, C.c_void_p, C.c_uint32, _f32p, C.c_size_t, C.c_uint32]),
        "s2r_set_voice_log": (C.c_int, [H, VOICE_LOG_FN, C.c_void_p]),
        "s2r_export_state": (C.c_int, [H, C.c_void_p]),
        "s2r_import_state": (C.c_int, [H, C.c_void_p]),
        "s2r_set_noise_seed": (C.c_int, [H, C.c_uint32, C.c_uint32]),
        "s2r_shard_voices": (C.c_uint32, [H]),
        "s2r_block_voices": (C.c_uint32, [H]),
        "s2r_device_count": (C.c_uint32, [H]),
        "s2r_double_release_count": (C.c_uint64, [H]),
        "s2r_set_timing": (C.c_int, [H, C.c_int]),
        "s2r_set_low_latency": (C.c_int, [H, C.c_int]),
        "s2r_low_latency_active": (C.c_int, [H]),
        "s2r_set_resident": (C.c_int, [H, C.c_int]),
        "s2r_resident_active": (C.c_int, [H]),
        "s2r_quiesce": (C.c_int, [H]),
        "s2r_exchange_create": (C.c_int, [H, C.c_uint32, C.c_void_p, C.c_size_t]),
        "s2r_exchange_attach": (C.c_int, [H, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
        "s2r_set_flat_shortcut": (C.c_int, [H, C.c_int]),
        "s2r_set_coeff_stream": (C.c_int, [H, C.c_int]),
        "s2r_set_uniform_window": (C.c_int, [H, C.c_int]),
        "s2r_uniform_window_chunks": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "s2r_last_render_ms": (C.c_float, [H]),
        "s2r_last_error": (C.c_char_p, [H]),
        "s2r_parse_patch_text": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(Patch), C.c_char_p, C.c_size_t]),
        "s2r_voice_pool_create": (H, [C.c_uint32]),
        "s2r_voice_pool_destroy": (None, [H]),
        "s2r_voice_pool_note_on": (C.c_uint32, [H, C.c_uint8, C.c_float]),
        "s2r_voice_pool_note_off": (C.c_int64, [H, C.c_uint8]),
        "s2r_voice_pool_advance": (None, [H, C.c_uint64]),
        "s2r_voice_pool_next_voice": (C.c_uint32, [H]),
        "s2r_voice_pool_set_threads": (None, [H, C.c_uint32, C.c_size_t]),
        "s2r_voice_pool_resolve": (C.c_uint32, [H, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
        "s2r_voice_pool_query": (C.c_int, [H, C.c_uint32, C.POINTER(VoiceState)]),
    }
    for name, (res, args) in sig.items():
        if _build.AB_LIB and not hasattr(L, name):               # (a library kept from an older build of these sources: A/B timing)
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    # s2r_fill once more, taking the buffer's address as an integer (Synth.sample)
    L._fill_raw = C.CFUNCTYPE(C.c_int, H, C.c_void_p, C.c_size_t, C.c_uint32)(("s2r_fill", L))
    _lib = L
    return L


def default_patch():
    """Synth::default_config() (synth.rs:125-152)"""
    p = Patch()
    load_library().s2r_default_patch(C.byref(p))
    return p


def parse_patch(text):
    """.synth2 text -> Patch (host only, no device needed)"""
    L = load_library()
    p = Patch()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    err = C.create_string_buffer(256)
    rc = L.s2r_parse_patch_text(raw, len(raw), C.byref(p), err, len(err))
    if rc != S2R_OK:
        raise S2rError(rc, err.value.decode())
    return p


def voice_pan(pan, key_spread, note):
    """the pan a note_on gives its voice under a program's pan and key spread (s2r_voice_pan; host only)"""
    return float(load_library().s2r_voice_pan(float(pan), float(key_spread), int(note)))


def pan_gains(p):
    """(gL, gR) of pan p: the constant-power law sqrt((1 -/+ p) / 2) in binary32 (s2r_pan_gains; host only)"""
    gl, gr = C.c_float(), C.c_float()
    load_library().s2r_pan_gains(float(p), C.byref(gl), C.byref(gr))
    return gl.value, gr.value


def voice_gain(level, velocity_sens, velocity):
    """the gain a note_on of `velocity` gives its voice under a program's level and velocity sensitivity (s2r_voice_gain; host only)"""
    return float(load_library().s2r_voice_gain(float(level), float(velocity_sens), float(velocity)))


def fader_gains(pan, w, fader, pan_shift):
    """(gL, gR) of a voice with pan `pan` and gain `w` under a program fader pair: the pan shifted and clamped, its
    constant-power gains times w, times the fader (s2r_fader_gains; host only)"""
    gl, gr = C.c_float(), C.c_float()
    load_library().s2r_fader_gains(float(pan), float(w), float(fader), float(pan_shift), C.byref(gl), C.byref(gr))
    return gl.value, gr.value


def send_gain(g, send):
    """the gain of a voice's aux send: g * send, one rounded binary32 multiply (s2r_send_gain; host only)"""
    return float(load_library().s2r_send_gain(float(g), float(send)))


def reverb_reference(ir, x_with_history, frames, dry, wet):
    """the bus reverb's rule for one channel on the host (s2r_reverb_reference): ir [K] float32, x_with_history K - 1 samples of
    history (oldest first) followed by `frames` dry samples; returns the `frames` output samples"""
    h = np.ascontiguousarray(ir, dtype=np.float32)
    x = np.ascontiguousarray(x_with_history, dtype=np.float32)
    frames = int(frames)
    if h.ndim != 1 or h.size < 1 or x.ndim != 1 or frames < 0 or x.size != h.size - 1 + frames:
        raise ValueError("reverb_reference: ir is [K] with K >= 1 and x_with_history holds K - 1 + frames samples")
    out = np.empty(frames, dtype=np.float32)
    rc = load_library().s2r_reverb_reference(h.ctypes.data_as(_f32p), h.size, x.ctypes.data_as(_f32p), frames, float(dry), float(wet),
                                             out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out


def delay_reference(delay_frames, feedback, cross, dry, wet, x, history):
    """the bus delay's rule for both channels on the host (s2r_delay_reference): x [frames, 2] float32 is the bus's signal, history
    [delay_frames, 2] the line's D frames in front of it, oldest first; returns (out [frames, 2], the history after the call
    [delay_frames, 2]).  `history` itself is left as it is."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = np.array(history, dtype=np.float32, order="C")
    d = int(delay_frames)
    if x.ndim != 2 or x.shape[1] != 2 or h.shape != (d, 2):
        raise ValueError("delay_reference: x is [frames, 2] and history is [delay_frames, 2]")
    out = np.empty_like(x)
    rc = load_library().s2r_delay_reference(d, float(feedback), float(cross), float(dry), float(wet), x.ctypes.data_as(_f32p), x.shape[0],
                                            h.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, h


def chorus_history_frames(base, depth):
    """H, the stereo frames of history a chorus of (base, depth) keeps: floor(float32(base + depth)) + 1, or 0 for a pair out of range
    (s2r_chorus_history_frames)"""
    return int(load_library().s2r_chorus_history_frames(float(base), float(depth)))


def chorus_rate(hz, sample_rate):
    """an LFO rate in Hz as a phase_inc: round(hz * 2^32 / sample_rate) modulo 2^32 (the spread of a chorus is in the same units:
    2^-32 turns)"""
    return int(round(float(hz) * 4294967296.0 / float(sample_rate))) & 0xFFFFFFFF


def chorus_reference(voices, base, depth, phase_inc, spread, dry, wet, x, history, phase):
    """the bus chorus's rule for both channels on the host (s2r_chorus_reference): x [frames, 2] float32 is the bus's signal, history
    [H, 2] the H frames of input in front of it, oldest first, phase the LFO's at frame 0; returns (out [frames, 2], the history after
    the call [H, 2], the phase after the call).  `history` itself is left as it is."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = np.array(history, dtype=np.float32, order="C")
    if x.ndim != 2 or x.shape[1] != 2 or h.ndim != 2 or h.shape[1] != 2:
        raise ValueError("chorus_reference: x is [frames, 2] and history is [H, 2]")
    hf = chorus_history_frames(base, depth)
    if hf and h.shape[0] != hf:                 # (a pair out of range is the library's to refuse)
        raise ValueError("chorus_reference: history is [chorus_history_frames(base, depth), 2]")
    out = np.empty_like(x)
    ph = C.c_uint32(int(phase) & 0xFFFFFFFF)
    rc = load_library().s2r_chorus_reference(int(voices), float(base), float(depth), int(phase_inc) & 0xFFFFFFFF, int(spread) & 0xFFFFFFFF, float(dry),
                                             float(wet), x.ctypes.data_as(_f32p), x.shape[0], h.ctypes.data_as(_f32p), C.byref(ph),
                                             out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, h, ph.value


def _eq_coeffs(coeffs, who):
    c = np.ascontiguousarray(coeffs, dtype=np.float32)
    if c.ndim == 1 and c.size == 5:
        c = c.reshape(1, 5)
    if c.ndim != 2 or c.shape[1] != 5 or c.shape[0] < 1:
        raise ValueError(who + ": coeffs is [n_bands, 5]: (b0, b1, b2, a1, a2) per band")
    return c


def eq_reference(coeffs, x, state):
    """the bus EQ's rule for both channels on the host (s2r_eq_reference): coeffs [n_bands, 5] float32 as (b0, b1, b2, a1, a2), x
    [frames, 2] float32 the bus's signal, state [n_bands, 4] as (s1_L, s1_R, s2_L, s2_R) per band; returns (out [frames, 2], the state
    after the call [n_bands, 4]).  `state` itself is left as it is."""
    c = _eq_coeffs(coeffs, "eq_reference")
    x = np.ascontiguousarray(x, dtype=np.float32)
    st = np.array(state, dtype=np.float32, order="C")
    if x.ndim != 2 or x.shape[1] != 2 or st.shape != (c.shape[0], 4):
        raise ValueError("eq_reference: x is [frames, 2] and state is [n_bands, 4]")
    out = np.empty_like(x)
    rc = load_library().s2r_eq_reference(c.shape[0], c.ctypes.data_as(_f32p), x.ctypes.data_as(_f32p), x.shape[0], st.ctypes.data_as(_f32p),
                                         out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, st


def eq_design(kind, freq_hz, gain_db, q, sample_rate):
    """a band (b0, b1, b2, a1, a2), float32 [5], from the usual parameters by the Audio-EQ-Cookbook formulas with q as Q
    (s2r_eq_design): kind one of EQ_PEAK, EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_LOWPASS, EQ_HIGHPASS; gain_db is the peak's and the shelves'"""
    out = np.empty(5, dtype=np.float32)
    rc = load_library().s2r_eq_design(int(kind), float(freq_hz), float(gain_db), float(q), float(sample_rate), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out


def _dyn_curve(curve, who):
    c = np.ascontiguousarray(curve, dtype=np.float32)
    if c.shape != (DYN_CURVE_POINTS,):
        raise ValueError(who + ": curve is [%d] float32" % DYN_CURVE_POINTS)
    return c


def dynamics_reference(curve, a_att, a_rel, key, x, y):
    """the bus dynamics' rule on the host (s2r_dynamics_reference): curve [DYN_CURVE_POINTS] float32, the two retention coefficients,
    key [frames, 2] float32 the key bus's signal (None: x keys itself), x [frames, 2] the bus's, y the gain carried in; returns (out
    [frames, 2], the gain after the call as np.float32, the minimum of the gain over the call — inf for no frames)"""
    c = _dyn_curve(curve, "dynamics_reference")
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = x if key is None else np.ascontiguousarray(key, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 2 or k.shape != x.shape:
        raise ValueError("dynamics_reference: key and x are [frames, 2]")
    out = np.empty_like(x)
    st = np.array([y], dtype=np.float32)
    mn = np.array([np.inf], dtype=np.float32)
    rc = load_library().s2r_dynamics_reference(c.ctypes.data_as(_f32p), C.c_float(float(np.float32(a_att))), C.c_float(float(np.float32(a_rel))),
                                               k.ctypes.data_as(_f32p), x.ctypes.data_as(_f32p), x.shape[0], st.ctypes.data_as(_f32p),
                                               out.ctypes.data_as(_f32p), mn.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, st[0], mn[0]


MULTIBAND_MAX_BANDS = 4                     # S2R_MULTIBAND_MAX_BANDS


def multiband_sections(n_bands):
    """S2R_MULTIBAND_SECTIONS: the crossover's sections per channel, 0, 4, 9, 15 for 1 .. 4 bands"""
    b = int(n_bands)
    return 4 * (b - 1) + (b - 1) * (b - 2) // 2


def multiband_state_floats(n_bands):
    """S2R_MULTIBAND_STATE: [section][s1_L, s1_R, s2_L, s2_R], then the bands' gains"""
    return 4 * multiband_sections(n_bands) + int(n_bands)


def multiband_design(sample_rate, splits_hz):
    """the crossover's rows for split frequencies strictly ascending inside (0, sample_rate / 2) (s2r_multiband_design): second-order
    Butterworth cookbook rows, float32 (lp [n, 5], hp [n, 5], ap [max(n - 1, 0), 5]) as (b0, b1, b2, a1, a2)"""
    f = np.ascontiguousarray(splits_hz, dtype=np.float64).reshape(-1)
    n = f.size
    lp, hp, ap = np.zeros((n, 5), np.float32), np.zeros((n, 5), np.float32), np.zeros((max(n - 1, 0), 5), np.float32)
    _rule_check(load_library().s2r_multiband_design(float(sample_rate), f.ctypes.data_as(C.POINTER(C.c_double)), n, _f32_or_null(lp),
                                                    _f32_or_null(hp), _f32_or_null(ap)))
    return lp, hp, ap


def _f32_or_null(a):
    return a.ctypes.data_as(_f32p) if a.size else None


def _multiband_args(who, coeffs, curves, attack, release):
    """(B, lp, hp, ap, curves, a_att, a_rel) as contiguous float32 arrays, B taken from the curves"""
    cv = np.ascontiguousarray(curves, dtype=np.float32)
    if cv.ndim != 2 or cv.shape[1] != DYN_CURVE_POINTS:
        raise ValueError(who + ": curves is [n_bands, %d] float32" % DYN_CURVE_POINTS)
    B = cv.shape[0]
    lp, hp, ap = (np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 5) for c in (coeffs if coeffs is not None else ((), (), ())))
    att, rel = np.ascontiguousarray(attack, dtype=np.float32).reshape(-1), np.ascontiguousarray(release, dtype=np.float32).reshape(-1)
    if lp.shape[0] != max(B - 1, 0) or hp.shape[0] != max(B - 1, 0) or ap.shape[0] != max(B - 2, 0) or att.size != B or rel.size != B:
        raise ValueError(who + ": %d curves need %d low-pass and high-pass rows, %d allpass rows and %d attack and release coefficients"
                         % (B, max(B - 1, 0), max(B - 2, 0), B))
    return B, lp, hp, ap, cv, att, rel


def multiband_reference(coeffs, curves, attack, release, x, state=None, want_bands=False):
    """the master multiband compressor's rule on the host (s2r_multiband_reference): coeffs (lp, hp, ap) as multiband_design returns
    them (None for one band), curves [B, DYN_CURVE_POINTS], the bands' retention coefficients, x [frames, 2] float32, state
    [multiband_state_floats(B)] (None: the state right after a set).  Returns (out [frames, 2], the state after the call, the bands'
    minima of y — inf for no frames) and, with want_bands, the band signals in front of the gains [B, frames, 2] as a fourth value"""
    B, lp, hp, ap, cv, att, rel = _multiband_args("multiband_reference", coeffs, curves, attack, release)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("multiband_reference: x is [frames, 2]")
    n_state = multiband_state_floats(B) if 1 <= B <= MULTIBAND_MAX_BANDS else 0
    if state is None:
        st = np.zeros(n_state, dtype=np.float32)
        if n_state:
            st[n_state - B:] = cv[:, 0]
    else:
        st = np.array(state, dtype=np.float32).reshape(-1)
        if st.size != n_state:
            raise ValueError("multiband_reference: the state is %d floats" % n_state)
    out, mn = np.empty_like(x), np.full(max(B, 1), np.inf, dtype=np.float32)
    bands = np.empty((B, x.shape[0], 2), dtype=np.float32) if want_bands else None
    _rule_check(load_library().s2r_multiband_reference(B, _f32_or_null(lp), _f32_or_null(hp), _f32_or_null(ap), cv.ctypes.data_as(_f32p), att.ctypes.data_as(_f32p),
                                                       rel.ctypes.data_as(_f32p), x.ctypes.data_as(_f32p), x.shape[0], st.ctypes.data_as(_f32p),
                                                       out.ctypes.data_as(_f32p), bands.ctypes.data_as(_f32p) if want_bands else None, mn.ctypes.data_as(_f32p)))
    return (out, st, mn[:B], bands) if want_bands else (out, st, mn[:B])


def dynamics_curve(threshold_db, ratio, knee_db=0.0, makeup_db=0.0):
    """the table [DYN_CURVE_POINTS] float32 of a soft-knee compressor (s2r_dynamics_curve): ratio in [1, inf], inf the limiter's curve"""
    out = np.empty(DYN_CURVE_POINTS, dtype=np.float32)
    rc = load_library().s2r_dynamics_curve(float(threshold_db), float(ratio), float(knee_db), float(makeup_db), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out


def dynamics_coef(ms, sample_rate):
    """the retention coefficient of a time constant (s2r_dynamics_coef): float32 exp(-1 / (ms * 0.001 * sample_rate)), 0 for ms == 0"""
    return np.float32(load_library().s2r_dynamics_coef(float(ms), float(sample_rate)))


def _room_delays(cd, ad, who):
    c = np.ascontiguousarray(cd, dtype=np.uint32)
    a = np.ascontiguousarray(ad, dtype=np.uint32)
    if c.shape != (ROOM_COMBS,) or a.shape != (ROOM_ALLPASSES,):
        raise ValueError(who + ": cd is [%d] and ad [%d] uint32" % (ROOM_COMBS, ROOM_ALLPASSES))
    return c, a


def _room_levels(feedback, damp, g, gain, dry, wet, cross):
    return [C.c_float(float(np.float32(v))) for v in (feedback, damp, g, gain, dry, wet, cross)]


def room_state_floats(cd, ad, spread):
    """the floats of a room's state (s2r_room_state_floats): 0 for delays out of range"""
    c, a = _room_delays(cd, ad, "room_state_floats")
    return int(load_library().s2r_room_state_floats(c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), int(spread)))


def room_reference(cd, ad, spread, feedback, damp, g, gain, dry, wet, cross, x, state=None):
    """the bus room's rule on the host (s2r_room_reference): cd [8] and ad [4] delays and the spread in frames, the seven levels, x
    [frames, 2] float32, state the flat float32 array of room_state_floats entries carried in (None: +0.0, as after a set); returns
    (out [frames, 2], the state after the call)"""
    c, a = _room_delays(cd, ad, "room_reference")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("room_reference: x is [frames, 2]")
    L = load_library()
    n = int(L.s2r_room_state_floats(c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), int(spread)))
    st = np.zeros(n, dtype=np.float32) if state is None else np.array(state, dtype=np.float32).ravel()
    if n and st.size != n:
        raise ValueError("room_reference: the state is %d floats, not %d" % (n, st.size))
    out = np.empty_like(x)
    rc = L.s2r_room_reference(c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), int(spread), *_room_levels(feedback, damp, g, gain, dry, wet, cross),
                              x.ctypes.data_as(_f32p), x.shape[0], st.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, L.s2r_status_string(rc).decode())
    return out, st


def room_design(sample_rate, size=1.0):
    """the public Freeverb tunings scaled by sample_rate / 44100 * size (s2r_room_design): (cd [8] uint32, ad [4] uint32, spread)"""
    c = np.empty(ROOM_COMBS, dtype=np.uint32)
    a = np.empty(ROOM_ALLPASSES, dtype=np.uint32)
    sp = C.c_uint32()
    rc = load_library().s2r_room_design(float(sample_rate), float(size), c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), C.byref(sp))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return c, a, sp.value


def _drive_curve(curve, who):
    c = np.ascontiguousarray(curve, dtype=np.float32)
    if c.shape != (DRIVE_CURVE_POINTS,):
        raise ValueError(who + ": curve is [%d] float32" % DRIVE_CURVE_POINTS)
    return c


def _f32(v):
    return C.c_float(float(np.float32(v)))


def drive_reference(curve, pre, dry, wet, x, history=None):
    """the bus drive's rule on the host (s2r_drive_reference): curve [DRIVE_CURVE_POINTS] float32, the three levels, x [frames, 2]
    float32, history [DRIVE_HISTORY, 2] float32 carried in (None: +0.0, as after a set); returns (out [frames, 2], the history after
    the call)"""
    c = _drive_curve(curve, "drive_reference")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("drive_reference: x is [frames, 2]")
    h = np.zeros((DRIVE_HISTORY, 2), dtype=np.float32) if history is None else np.array(history, dtype=np.float32)
    if h.shape != (DRIVE_HISTORY, 2):
        raise ValueError("drive_reference: the history is [%d, 2]" % DRIVE_HISTORY)
    out = np.empty_like(x)
    L = load_library()
    rc = L.s2r_drive_reference(c.ctypes.data_as(_f32p), _f32(pre), _f32(dry), _f32(wet), x.ctypes.data_as(_f32p), x.shape[0], h.ctypes.data_as(_f32p),
                               out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, L.s2r_status_string(rc).decode())
    return out, h


def drive_curve(kind, amount=1.0):
    """a table [DRIVE_CURVE_POINTS] float32 by design (s2r_drive_curve): DRIVE_LINEAR, DRIVE_TANH, DRIVE_HARD, DRIVE_CUBIC or DRIVE_FOLD
    at `amount`, the gain in front of the shape"""
    out = np.empty(DRIVE_CURVE_POINTS, dtype=np.float32)
    rc = load_library().s2r_drive_curve(int(kind), float(amount), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out


def drive_taps():
    """the library's prototype filter h [DRIVE_TAPS] float32 (s2r_drive_taps): the decimator's taps; the interpolator's are 4 h"""
    out = np.empty(DRIVE_TAPS, dtype=np.float32)
    rc = load_library().s2r_drive_taps(out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out


def flanger_history_frames(base, depth):
    """H, the stereo frames of its line signal a flanger of (base, depth) keeps: floor(float32(base + depth)) + 1, or 0 for a pair out
    of range (s2r_flanger_history_frames)"""
    return int(load_library().s2r_flanger_history_frames(float(base), float(depth)))


def flanger_reference(base, depth, phase_inc, spread, feedback, cross, dry, wet, x, history, phase):
    """the bus flanger's rule on the host (s2r_flanger_reference): x [frames, 2] float32 is the bus's signal, history [H, 2] the last H
    frames of the stage's line signal w, oldest first, phase the LFO's at frame 0; returns (out [frames, 2], the history after the call
    [H, 2], the phase after the call).  `history` itself is left as it is."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = np.array(history, dtype=np.float32, order="C")
    if x.ndim != 2 or x.shape[1] != 2 or h.ndim != 2 or h.shape[1] != 2:
        raise ValueError("flanger_reference: x is [frames, 2] and history is [H, 2]")
    hf = flanger_history_frames(base, depth)
    if hf and h.shape[0] != hf:                 # (a pair out of range is the library's to refuse)
        raise ValueError("flanger_reference: history is [flanger_history_frames(base, depth), 2]")
    out = np.empty_like(x)
    ph = C.c_uint32(int(phase) & 0xFFFFFFFF)
    rc = load_library().s2r_flanger_reference(float(base), float(depth), int(phase_inc) & 0xFFFFFFFF, int(spread) & 0xFFFFFFFF, float(feedback),
                                              float(cross), float(dry), float(wet), x.ctypes.data_as(_f32p), x.shape[0], h.ctypes.data_as(_f32p),
                                              C.byref(ph), out.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, h, ph.value


def master_reference(stems, r0, r1, m0, m1):
    """the master section's rule on the host (s2r_master_reference): stems [n_buses, frames, 2] float32, r0 / r1 [n_buses] the returns'
    applied and target levels, m0 / m1 the master fader's; returns (master [frames, 2], peak [n_buses + 1, 2], energy [n_buses + 1, 2])"""
    y = np.ascontiguousarray(stems, dtype=np.float32)
    a = np.ascontiguousarray(r0, dtype=np.float32)
    b = np.ascontiguousarray(r1, dtype=np.float32)
    if y.ndim != 3 or y.shape[2] != 2 or a.shape != (y.shape[0],) or b.shape != (y.shape[0],):
        raise ValueError("master_reference: stems is [n_buses, frames, 2], r0 and r1 are [n_buses]")
    n_buses, frames = y.shape[0], y.shape[1]
    out = np.empty((frames, 2), dtype=np.float32)
    peak = np.empty((n_buses + 1, 2), dtype=np.float32)
    energy = np.empty((n_buses + 1, 2), dtype=np.float32)
    rc = load_library().s2r_master_reference(y.ctypes.data_as(_f32p), n_buses, frames, a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p),
                                             float(m0), float(m1), out.ctypes.data_as(_f32p), peak.ctypes.data_as(_f32p),
                                             energy.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return out, peak, energy


def limiter_reference(x, ceiling, lookahead, hold, xh=None, gh=None):
    """the master limiter's rule on the host (s2r_limiter_reference): x [frames, 2] float32; xh [lookahead, 2] and gh
    [2 * lookahead + hold] the state the call starts from (None: the initial state).  Returns (y [frames, 2], gain [frames], xh, gh)
    with the state the call leaves; the arguments are not modified."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L, Hd = int(lookahead), int(hold)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("limiter_reference: x is [frames, 2]")
    xh = np.zeros((max(L, 0), 2), dtype=np.float32) if xh is None else np.array(xh, dtype=np.float32, order="C")
    gh = np.ones(max(2 * L + Hd, 0), dtype=np.float32) if gh is None else np.array(gh, dtype=np.float32, order="C")
    if 0 < L <= LIMITER_MAX_LOOKAHEAD and 0 <= Hd <= LIMITER_MAX_HOLD and (xh.shape != (L, 2) or gh.shape != (2 * L + Hd,)):
        raise ValueError("limiter_reference: xh is [lookahead, 2], gh is [2 * lookahead + hold]")
    frames = x.shape[0]
    y = np.empty((frames, 2), dtype=np.float32)
    gain = np.empty(frames, dtype=np.float32)
    rc = load_library().s2r_limiter_reference(x.ctypes.data_as(_f32p), frames, float(ceiling), max(L, 0), max(Hd, 0), xh.ctypes.data_as(_f32p),
                                              gh.ctypes.data_as(_f32p), y.ctypes.data_as(_f32p), gain.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return y, gain, xh, gh


def limiter_tp_reference(x, ceiling, lookahead, hold, xh=None, gh=None):
    """the master limiter's rule with the true-peak detector on the host (s2r_limiter_tp_reference): as limiter_reference, with xh
    [lookahead + LIMITER_TP_HISTORY, 2].  Returns (y [frames, 2], gain [frames], xh, gh); y is x delayed by lookahead +
    LIMITER_TP_LATENCY frames times the gain; the arguments are not modified."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L, Hd = int(lookahead), int(hold)
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("limiter_tp_reference: x is [frames, 2]")
    xh = np.zeros((max(L, 0) + LIMITER_TP_HISTORY, 2), dtype=np.float32) if xh is None else np.array(xh, dtype=np.float32, order="C")
    gh = np.ones(max(2 * L + Hd, 0), dtype=np.float32) if gh is None else np.array(gh, dtype=np.float32, order="C")
    if 0 < L <= LIMITER_MAX_LOOKAHEAD and 0 <= Hd <= LIMITER_MAX_HOLD and (xh.shape != (L + LIMITER_TP_HISTORY, 2) or gh.shape != (2 * L + Hd,)):
        raise ValueError("limiter_tp_reference: xh is [lookahead + 16, 2], gh is [2 * lookahead + hold]")
    frames = x.shape[0]
    y = np.empty((frames, 2), dtype=np.float32)
    gain = np.empty(frames, dtype=np.float32)
    rc = load_library().s2r_limiter_tp_reference(x.ctypes.data_as(_f32p), frames, float(ceiling), max(L, 0), max(Hd, 0), xh.ctypes.data_as(_f32p),
                                                 gh.ctypes.data_as(_f32p), y.ctypes.data_as(_f32p), gain.ctypes.data_as(_f32p))
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())
    return y, gain, xh, gh


def _rule_check(rc):
    if rc != S2R_OK:
        raise S2rError(rc, load_library().s2r_status_string(rc).decode())


def loudness_design(sample_rate=48000.0):
    """BS.1770's K-weighting pre-filter at `sample_rate` (s2r_loudness_design): [2, 5] float32, the high shelf and the high-pass, each
    (b0, b1, b2, a1, a2)"""
    c = np.empty((2, 5), dtype=np.float32)
    _rule_check(load_library().s2r_loudness_design(float(sample_rate), c.ctypes.data_as(_f32p)))
    return c


def loudness_reference(coeffs, hop, stems, master, state=None, pos=0):
    """the loudness meter's device rule on the host (s2r_loudness_reference): stems [n_buses, frames, 2] float32 (None: no buses),
    master [frames, 2]; state [LOUDNESS_STATE] and pos what the call starts from (None: the initial state).  Returns (rows [k, 18] —
    the hops the call completes —, state, pos, true_peak [2]); the arguments are not modified."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
    master = np.ascontiguousarray(master, dtype=np.float32)
    if coeffs.size != 10 or master.ndim != 2 or master.shape[1] != 2:
        raise ValueError("loudness_reference: coeffs is [2, 5], master is [frames, 2]")
    frames = master.shape[0]
    if stems is None:
        stems = np.zeros((0, frames, 2), dtype=np.float32)
    stems = np.ascontiguousarray(stems, dtype=np.float32)
    if stems.ndim != 3 or stems.shape[1:] != (frames, 2):
        raise ValueError("loudness_reference: stems is [n_buses, frames, 2]")
    state = np.zeros(LOUDNESS_STATE, dtype=np.float32) if state is None else np.array(state, dtype=np.float32, order="C").reshape(-1)
    if state.size != LOUDNESS_STATE:
        raise ValueError("loudness_reference: state is [LOUDNESS_STATE]")
    hop, at = int(hop), C.c_uint32(int(pos))
    cap = (frames // max(hop, LOUDNESS_MIN_HOP) + 1) * LOUDNESS_CHANNELS
    rows, n, tp = np.zeros(cap, dtype=np.float32), C.c_size_t(0), np.zeros(2, dtype=np.float32)
    _rule_check(load_library().s2r_loudness_reference(coeffs.ctypes.data_as(_f32p), hop, stems.ctypes.data_as(_f32p) if stems.shape[0] else None,
                                                      stems.shape[0], master.ctypes.data_as(_f32p), frames, state.ctypes.data_as(_f32p), C.byref(at),
                                                      rows.ctypes.data_as(_f32p), rows.size, C.byref(n), tp.ctypes.data_as(_f32p)))
    return rows[:n.value * LOUDNESS_CHANNELS].reshape(-1, LOUDNESS_CHANNELS).copy(), state, at.value, tp


def loudness_readings(rows, hop, programme):
    """(momentary, short-term, integrated) in LKFS of one programme from hop rows [n_hops, 18] (s2r_loudness_readings): binary64, -inf
    where there is too little data or nothing passes the gates"""
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, LOUDNESS_CHANNELS)
    out = (C.c_double * 3)()
    _rule_check(load_library().s2r_loudness_readings(rows.ctypes.data_as(_f32p) if rows.shape[0] else None, rows.shape[0], int(hop), int(programme), out))
    return out[0], out[1], out[2]


def _dither_arg(kind):
    k = _DITHER_KINDS.get(kind.lower(), -1) if isinstance(kind, str) else int(kind)
    if k < 0:
        raise ValueError("dither is one of %s" % sorted(_DITHER_KINDS))
    return k


def pcm_shaper(kind):
    """the error-feedback taps of shaper `kind` (a SHAPER_* value, 0 .. 5; s2r_pcm_shaper): float32 [n_taps]"""
    taps, n = np.empty(PCM_MAX_TAPS, dtype=np.float32), C.c_uint32()
    _rule_check(load_library().s2r_pcm_shaper(int(kind), taps.ctypes.data_as(_f32p), C.byref(n)))
    return taps[:n.value].copy()


def _shaper_arg(shaper):
    if np.isscalar(shaper):
        return pcm_shaper(shaper)
    return np.ascontiguousarray(shaper, dtype=np.float32).reshape(-1)


def pcm_dither(seed, t, q, kind="tpdf"):
    """the PCM stage's dither of frame `t` and channel `q` in LSB (s2r_pcm_dither): a float"""
    d = C.c_float()
    _rule_check(load_library().s2r_pcm_dither(int(seed) & 0xffffffff, int(t) & 0xffffffff, int(q), _dither_arg(kind), C.byref(d)))
    return d.value


def pcm_pack(pcm, bits, bytes_per_sample):
    """samples of `bits` bits into little-endian containers of 2, 3 or 4 bytes, left-justified (s2r_pcm_pack): uint8 [pcm.size *
    bytes_per_sample], in the samples' C order"""
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    out = np.zeros(pcm.size * max(int(bytes_per_sample), 0), dtype=np.uint8)
    _rule_check(load_library().s2r_pcm_pack(pcm.ctypes.data_as(C.POINTER(C.c_int32)), pcm.size, int(bits), int(bytes_per_sample),
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def pcm_reference(stems, master, bits=16, dither="tpdf", shaper=0, seed=0, state=None, t=0):
    """the PCM stage's device rule on the host (s2r_pcm_reference): stems [n_buses, frames, 2] float32 (None: no buses), master
    [frames, 2]; state [18, 9] and t what the call starts from (None: the initial state).  Returns (pcm int32 [9, frames, 2], state,
    t, clips uint32 [18]); the arguments are not modified."""
    taps = _shaper_arg(shaper)
    master = np.ascontiguousarray(master, dtype=np.float32)
    if master.ndim != 2 or master.shape[1] != 2:
        raise ValueError("pcm_reference: master is [frames, 2]")
    frames = master.shape[0]
    if stems is None:
        stems = np.zeros((0, frames, 2), dtype=np.float32)
    stems = np.ascontiguousarray(stems, dtype=np.float32)
    if stems.ndim != 3 or stems.shape[1:] != (frames, 2):
        raise ValueError("pcm_reference: stems is [n_buses, frames, 2]")
    state = np.zeros(PCM_STATE, dtype=np.float32) if state is None else np.array(state, dtype=np.float32, order="C").reshape(-1)
    if state.size != PCM_STATE:
        raise ValueError("pcm_reference: state is [18, 9]")
    at = C.c_uint32(int(t) & 0xffffffff)
    pcm, clips = np.zeros((PCM_PROGRAMMES, frames, 2), dtype=np.int32), np.zeros(PCM_CHANNELS, dtype=np.uint32)
    _rule_check(load_library().s2r_pcm_reference(int(bits), _dither_arg(dither), taps.ctypes.data_as(_f32p) if taps.size else None, taps.size, int(seed) & 0xffffffff,
                                                 stems.ctypes.data_as(_f32p) if stems.shape[0] else None, stems.shape[0], master.ctypes.data_as(_f32p), frames,
                                                 state.ctypes.data_as(_f32p), C.byref(at), pcm.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 clips.ctypes.data_as(C.POINTER(C.c_uint32))))
    return pcm, state.reshape(PCM_CHANNELS, PCM_MAX_TAPS), at.value, clips


def resampler_state_floats(T):
    """S2R_RESAMPLER_STATE(T): 18 rows of T - 1 frames"""
    return RESAMPLER_CHANNELS * (int(T) - 1)


def resampler_max_out(frames, L, M):
    """S2R_RESAMPLER_MAX_OUT: the most output frames of a call of `frames` frames"""
    return (int(frames) * int(L) + int(M) - 1) // int(M) + 1


def resampler_count(L, M, ph, frames):
    """the output frames of a call of `frames` frames that starts at position ph (s2r_resampler_count)"""
    n = C.c_size_t()
    _rule_check(load_library().s2r_resampler_count(int(L), int(M), int(ph), int(frames), C.byref(n)))
    return n.value


def resampler_design(L, M, T, beta=10.0, rolloff=0.9):
    """a Kaiser-windowed sinc for the ratio L / M with T taps a phase (s2r_resampler_design): float32 [L, T], every row of sum 1"""
    table = np.zeros((max(int(L), 0), max(int(T), 0)), dtype=np.float32)
    _rule_check(load_library().s2r_resampler_design(int(L), int(M), int(T), float(beta), float(rolloff), table.ctypes.data_as(_f32p)))
    return table


def resampler_reference(stems, master, L, M, table, state=None, ph=0):
    """the resampler's device rule on the host (s2r_resampler_reference): stems [n_buses, frames, 2] float32 (None: no buses), master
    [frames, 2]; table [L, T]; state [18, T - 1] and ph what the call starts from (None: the initial state).  Returns (out float32
    [9, count, 2], state, ph); the arguments are not modified."""
    table = np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 2:
        raise ValueError("resampler_reference: table is [L, T]")
    T = table.shape[1]
    master = np.ascontiguousarray(master, dtype=np.float32)
    if master.ndim != 2 or master.shape[1] != 2:
        raise ValueError("resampler_reference: master is [frames, 2]")
    frames = master.shape[0]
    if stems is None:
        stems = np.zeros((0, frames, 2), dtype=np.float32)
    stems = np.ascontiguousarray(stems, dtype=np.float32)
    if stems.ndim != 3 or stems.shape[1:] != (frames, 2):
        raise ValueError("resampler_reference: stems is [n_buses, frames, 2]")
    n_state = max(resampler_state_floats(T), 0)
    state = np.zeros(n_state, dtype=np.float32) if state is None else np.array(state, dtype=np.float32, order="C").reshape(-1)
    if state.size != n_state or table.shape[0] != int(L):
        raise ValueError("resampler_reference: table is [L, T] and state [18, T - 1]")
    cap = resampler_max_out(frames, L, max(int(M), 1))
    out, at, n = np.zeros((RESAMPLER_PROGRAMMES, cap, 2), dtype=np.float32), C.c_uint32(int(ph)), C.c_size_t()
    _rule_check(load_library().s2r_resampler_reference(int(L), int(M), T, table.ctypes.data_as(_f32p), stems.ctypes.data_as(_f32p) if stems.shape[0] else None,
                                                       stems.shape[0], master.ctypes.data_as(_f32p), frames, state.ctypes.data_as(_f32p), C.byref(at),
                                                       out.ctypes.data_as(_f32p), cap, C.byref(n)))
    return out[:, :n.value].copy(), state.reshape(RESAMPLER_CHANNELS, T - 1), at.value


def spectrum_window(kind, n_fft):
    """the periodic window `kind` ('rect', 'hann', 'hamming', 'blackman-harris' or a WINDOW_* value) of n_fft points
    (s2r_spectrum_window): float32 [n_fft]"""
    k = _WINDOW_KINDS.get(kind.lower(), -1) if isinstance(kind, str) else int(kind)
    if k < 0:
        raise ValueError("spectrum_window: kind is one of %s" % sorted(_WINDOW_KINDS))
    w = np.empty(max(int(n_fft), 0), dtype=np.float32)
    _rule_check(load_library().s2r_spectrum_window(k, int(n_fft), w.ctypes.data_as(_f32p)))
    return w


def spectrum_twiddles(n_fft):
    """the spectrum meter's twiddle table (s2r_spectrum_twiddles): float32 [n_fft / 2, 2], (re, im)"""
    t = np.empty((max(int(n_fft), 0) // 2, 2), dtype=np.float32)
    _rule_check(load_library().s2r_spectrum_twiddles(int(n_fft), t.ctypes.data_as(_f32p)))
    return t


def _spectrum_window_arg(window, n_fft):
    if isinstance(window, str) or np.isscalar(window):
        return spectrum_window(window, n_fft)
    w = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
    if w.size != int(n_fft):
        raise ValueError("the window holds n_fft values")
    return w


def spectrum_reference(n_fft, hop, window, stems, master, state=None, pos=0):
    """the spectrum meter's device rule on the host (s2r_spectrum_reference): stems [n_buses, frames, 2] float32 (None: no buses),
    master [frames, 2]; state [9, n_fft, 2] and pos what the call starts from (None: the initial state).  Returns (rows
    [k, 9, n_fft / 2 + 1] — the rows the call completes —, state, pos); the arguments are not modified."""
    n_fft, hop = int(n_fft), int(hop)
    window = _spectrum_window_arg(window, n_fft)
    master = np.ascontiguousarray(master, dtype=np.float32)
    if master.ndim != 2 or master.shape[1] != 2:
        raise ValueError("spectrum_reference: master is [frames, 2]")
    frames = master.shape[0]
    if stems is None:
        stems = np.zeros((0, frames, 2), dtype=np.float32)
    stems = np.ascontiguousarray(stems, dtype=np.float32)
    if stems.ndim != 3 or stems.shape[1:] != (frames, 2):
        raise ValueError("spectrum_reference: stems is [n_buses, frames, 2]")
    state = np.zeros(18 * n_fft, dtype=np.float32) if state is None else np.array(state, dtype=np.float32, order="C").reshape(-1)
    if state.size != 18 * n_fft:
        raise ValueError("spectrum_reference: state is [9, n_fft, 2]")
    bins, at = n_fft // 2 + 1, C.c_uint32(int(pos))
    cap = ((int(pos) + frames) // max(hop, 1) + 1) * SPECTRUM_PROGRAMMES * bins
    rows, n = np.zeros(cap, dtype=np.float32), C.c_size_t(0)
    _rule_check(load_library().s2r_spectrum_reference(n_fft, hop, window.ctypes.data_as(_f32p), stems.ctypes.data_as(_f32p) if stems.shape[0] else None,
                                                      stems.shape[0], master.ctypes.data_as(_f32p), frames, state.ctypes.data_as(_f32p), C.byref(at),
                                                      rows.ctypes.data_as(_f32p), rows.size, C.byref(n)))
    return rows[:n.value * SPECTRUM_PROGRAMMES * bins].reshape(-1, SPECTRUM_PROGRAMMES, bins).copy(), state.reshape(SPECTRUM_PROGRAMMES, n_fft, 2), at.value


def _spectrum_rows_arg(rows, n_fft):
    bins = int(n_fft) // 2 + 1
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if bins < 2 or rows.size % (SPECTRUM_PROGRAMMES * bins):
        raise ValueError("the rows are [n_rows, 9, n_fft / 2 + 1]")
    return rows.reshape(-1, SPECTRUM_PROGRAMMES, bins)


def spectrum_readings(rows, window, programme, n_avg=1):
    """dB per bin of one programme over the last n_avg of rows [n_rows, 9, n_fft / 2 + 1] (s2r_spectrum_readings): float64
    [n_fft / 2 + 1]; 0 dB is a bin-centred sine of amplitude 1 on both channels; silence reads -inf"""
    window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
    rows = _spectrum_rows_arg(rows, window.size)
    out = np.empty(window.size // 2 + 1, dtype=np.float64)
    _rule_check(load_library().s2r_spectrum_readings(rows.ctypes.data_as(_f32p) if rows.shape[0] else None, rows.shape[0], window.size,
                                                     window.ctypes.data_as(_f32p), int(programme), int(n_avg), out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
    return out


def spectrum_band_readings(rows, window, programme, sample_rate, bands_per_octave, n_avg=1):
    """(dB [n_bands], centres in Hz [n_bands]) of one programme over the last n_avg rows (s2r_spectrum_band_readings)"""
    window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
    rows = _spectrum_rows_arg(rows, window.size)
    cap = 256
    db, fc, n = np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.float64), C.c_size_t(0)
    dp = C.POINTER(C.c_double)
    _rule_check(load_library().s2r_spectrum_band_readings(rows.ctypes.data_as(_f32p) if rows.shape[0] else None, rows.shape[0], window.size,
                                                          window.ctypes.data_as(_f32p), int(programme), int(n_avg), float(sample_rate), int(bands_per_octave),
                                                          db.ctypes.data_as(dp), fc.ctypes.data_as(dp), cap, C.byref(n)))
    return db[:n.value].copy(), fc[:n.value].copy()


def stream_frame_json(samples):
    """one buffer as the text frame of the reference's websocket audio server (threads.rs:303-305):
    serde_json's rendering of a Vec<f32> (host only, no device needed)"""
    L = load_library()
    a = np.ascontiguousarray(samples, dtype=np.float32)
    cap = L.s2r_stream_frame_json(None, a.size, None, 0)      # the worst case for n samples (3 + 18 n)
    buf = C.create_string_buffer(cap)
    n = L.s2r_stream_frame_json(a.ctypes.data_as(C.c_void_p), a.size, buf, cap)
    return buf.raw[:n].decode("ascii")


def shard_pool_indices(total_voices, shard_index, shard_count, interleave):
    """pool indices of a round-robin shard's local voices, in local order (s2r_config.shard_interleave)"""
    local = np.arange(total_voices // shard_count)
    return ((local // interleave) * shard_count + shard_index) * interleave + local % interleave


class VoicePool:
    """The allocation policy of Synth (synth.rs:61-120) without a device."""

    def __init__(self, total_voices):
        self.L = load_library()
        self.p = self.L.s2r_voice_pool_create(total_voices)
        if not self.p:
            raise MemoryError("s2r_voice_pool_create")

    def __del__(self):
        if getattr(self, "p", None):
            self.L.s2r_voice_pool_destroy(self.p)
            self.p = None

    def note_on(self, note, velocity=1.0):
        return self.L.s2r_voice_pool_note_on(self.p, note, velocity)

    def note_off(self, note):
        return self.L.s2r_voice_pool_note_off(self.p, note)

    def advance(self, frames):
        self.L.s2r_voice_pool_advance(self.p, frames)

    def set_threads(self, worker_threads, batch_threshold=4096):
        self.L.s2r_voice_pool_set_threads(self.p, worker_threads, batch_threshold)

    def resolve(self, events, frames_moved=0):
        """the batch form: (voice per event, frame of the last event)"""
        ev = np.ascontiguousarray(events, dtype=NOTE_EVENT_DTYPE)
        out = np.empty(ev.size, dtype=np.int64)
        t = self.L.s2r_voice_pool_resolve(self.p, ev.ctypes.data, ev.size, frames_moved, out.ctypes.data)
        return out, int(t)

    def next_voice(self):
        return self.L.s2r_voice_pool_next_voice(self.p)

    def query(self, i):
        st = VoiceState()
        rc = self.L.s2r_voice_pool_query(self.p, i, C.byref(st))
        if rc != S2R_OK:
            raise S2rError(rc, "voice pool query")
        return st


class Synth:
    """``s2_lib::try3::synth::Synth`` on an MI355X.

    ``num_voices`` replaces the reference's ``NUM_VOICES = 8`` (synth.rs:7).  ``devices=[d0, d1, ...]``: ONE Synth over
    several GPUs (s2r_config.devices: the pool cut into one shard per device, the allocation policy run once, the
    shards' partial mixes added in shard order on d0).  With one process per GPU instead (torch.distributed,
    synth2_amd/sharded.py) every rank builds a Synth over the same pool with its own ``shard_begin`` /
    ``shard_voices`` (or ``shard_interleave`` / ``shard_index`` / ``shard_count``) and feeds it the same note events.
    """

    def __init__(self, num_voices=8, max_frames=2048, device=-1, shard_begin=0, shard_voices=0,
                 block_voices=0, mix_groups=0, shard_interleave=0, shard_index=0, shard_count=1, devices=None):
        self.L = load_library()
        self.h = C.c_void_p()
        devs = list(devices) if devices is not None else []
        if len(devs) > 16:
            raise ValueError("a device list holds at most 16 devices")
        cfg = Config(C.sizeof(Config), num_voices, shard_begin, shard_voices, max_frames, device, block_voices, mix_groups,
                     0, shard_interleave, shard_index, shard_count, len(devs), (C.c_int32 * 16)(*devs))
        rc = self.L.s2r_create(C.byref(cfg), C.byref(self.h))
        if rc != S2R_OK:
            self.h = None
            raise S2rError(rc, self.L.s2r_status_string(rc).decode())
        self.num_voices = num_voices
        self.max_frames = max_frames
        self.shard_voices = self.L.s2r_shard_voices(self.h)
        self.block_voices = self.L.s2r_block_voices(self.h)
        self.device_count = self.L.s2r_device_count(self.h)
        self._fill_raw = self.L._fill_raw

    # Synth::new() (synth.rs:54-59)
    @classmethod
    def new(cls):
        return cls()

    def close(self):
        if getattr(self, "h", None):
            self.L.s2r_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != S2R_OK:
            raise S2rError(rc, self.L.s2r_last_error(self.h).decode() or self.L.s2r_status_string(rc).decode())

    # --- patch ---
    def load_patch(self, text):
        raw = text.encode() if isinstance(text, str) else bytes(text)
        self._check(self.L.s2r_load_patch(self.h, raw, len(raw)))

    def set_patch(self, patch):
        self._check(self.L.s2r_set_patch(self.h, C.byref(patch)))

    def set_patch_bank(self, patches):
        """1..256 patches; the current program picks the one a note_on gives its voice"""
        arr = (Patch * len(patches))(*patches)
        self._check(self.L.s2r_set_patch_bank(self.h, arr, len(patches)))

    @property
    def patch_bank_size(self):
        return self.L.s2r_patch_bank_size(self.h)

    def program_change(self, program):
        self._check(self.L.s2r_program_change(self.h, int(program)))

    def get_patch(self):
        p = Patch()
        self._check(self.L.s2r_get_patch(self.h, C.byref(p)))
        return p

    # --- events (synth.rs:61-80) ---
    def note_on(self, note, velocity=Velocity(1.0)):
        idx = C.c_uint32()
        self._check(self.L.s2r_note_on_ex(self.h, int(note), float(velocity), C.byref(idx)))
        return idx.value

    def note_off(self, note):
        self._check(self.L.s2r_note_off(self.h, int(note)))

    def note_events(self, events):
        """A batch of events (structured array NOTE_EVENT_DTYPE: kind 1=on 0=off, note, velocity),
        applied in order in one call — s2_bin's apply_all_midi_messages (main.rs:170-187)."""
        ev = np.ascontiguousarray(events, dtype=NOTE_EVENT_DTYPE)
        self._check(self.L.s2r_note_events(self.h, ev.ctypes.data, ev.size))

    # --- Synth::sample(&mut [f32], SampleRateKhz) (synth.rs:154-169) ---
    def sample(self, buffer, sample_rate=SampleRateKhz(48000)):
        """Overwrites ``buffer`` (1-D float32, C-contiguous) and returns it."""
        if isinstance(buffer, int):
            buffer = np.empty(buffer, dtype=np.float32)
        assert buffer.dtype == np.float32 and buffer.flags["C_CONTIGUOUS"] and buffer.ndim == 1
        # (the array's address without building a ctypes view of it: a microsecond per call that a 16-frame fill notices)
        rc = self._fill_raw(self.h, buffer.__array_interface__["data"][0], buffer.size, int(sample_rate))
        if rc:
            self._check(rc)
        return buffer

    def sample_begin(self, frames, sample_rate=SampleRateKhz(48000)):
        """first half of sample(): queue the fill (at most two in flight, like s2_bin's two buffers)"""
        self._check(self.L.s2r_fill_begin(self.h, int(frames), int(sample_rate)))

    def sample_end(self, buffer):
        """second half: wait for the oldest fill in flight and copy it into ``buffer``"""
        assert buffer.dtype == np.float32 and buffer.flags["C_CONTIGUOUS"] and buffer.ndim == 1
        self._check(self.L.s2r_fill_end(self.h, buffer.ctypes.data_as(_f32p), buffer.size))
        return buffer

    @property
    def pending_frames(self):
        """frames of the oldest fill begun and not yet ended (0: none in flight)"""
        return int(self.L.s2r_fill_pending_frames(self.h))

    def sample_oversampled(self, frames, sample_rate=SampleRateKhz(48000)):
        """build-defined 4x oversampling: rendered at 4 * sample_rate, decimated to `frames` samples"""
        out = np.empty(frames, dtype=np.float32)
        self._check(self.L.s2r_fill_oversampled(self.h, out.ctypes.data_as(_f32p), frames, int(sample_rate)))
        return out

    def sample_stereo(self, frames, sample_rate=SampleRateKhz(48000)):
        out = np.empty(2 * frames, dtype=np.float32)
        self._check(self.L.s2r_fill_stereo(self.h, out.ctypes.data_as(_f32p), frames, int(sample_rate)))
        return out.reshape(frames, 2)

    # --- true stereo (build-defined; s2r.h: s2r_fill_panned) ---
    def set_program_pan(self, program, pan, key_spread=0.0):
        """pan and key spread (both in [-1, 1]) of a bank program: what a note_on under that program gives its voice"""
        self._check(self.L.s2r_set_program_pan(self.h, int(program), float(pan), float(key_spread)))

    def get_program_pan(self, program):
        pan, spread = C.c_float(), C.c_float()
        self._check(self.L.s2r_get_program_pan(self.h, int(program), C.byref(pan), C.byref(spread)))
        return pan.value, spread.value

    def voice_pans(self):
        """every shard voice's pan, local order (the checkpoint companion of export_state)"""
        out = np.empty(self.shard_voices, dtype=np.float32)
        self._check(self.L.s2r_get_voice_pans(self.h, out.ctypes.data_as(_f32p)))
        return out

    def set_voice_pans(self, pans):
        arr = np.ascontiguousarray(pans, dtype=np.float32)
        assert arr.size == self.shard_voices
        self._check(self.L.s2r_set_voice_pans(self.h, arr.ctypes.data_as(_f32p)))

    def sample_panned(self, frames, sample_rate=SampleRateKhz(48000)):
        """the panned two-channel mixdown: (frames, 2) float32, columns L and R"""
        out = np.empty(2 * frames, dtype=np.float32)
        self._check(self.L.s2r_fill_panned(self.h, out.ctypes.data_as(_f32p), frames, int(sample_rate)))
        return out.reshape(frames, 2)

    # --- the voice mixer (build-defined; s2r.h: s2r_fill_buses) ---
    def set_program_mix(self, program, level=1.0, velocity_sens=0.0, bus=0):
        """level and velocity sensitivity (both in [0, 1]) and output bus (below MAX_BUSES) of a bank program: what a note_on under
        that program gives its voice.  Only sample_buses applies them."""
        self._check(self.L.s2r_set_program_mix(self.h, int(program), float(level), float(velocity_sens), int(bus)))

    def get_program_mix(self, program):
        level, sens, bus = C.c_float(), C.c_float(), C.c_uint32()
        self._check(self.L.s2r_get_program_mix(self.h, int(program), C.byref(level), C.byref(sens), C.byref(bus)))
        return level.value, sens.value, bus.value

    def voice_mix(self):
        """(gains float32, buses uint8) of every shard voice, local order (checkpoint companions of export_state and voice_pans)"""
        gains = np.empty(self.shard_voices, dtype=np.float32)
        buses = np.empty(self.shard_voices, dtype=np.uint8)
        self._check(self.L.s2r_get_voice_mix(self.h, gains.ctypes.data_as(_f32p), buses.ctypes.data_as(C.POINTER(C.c_uint8))))
        return gains, buses

    def set_voice_mix(self, gains, buses):
        g = np.ascontiguousarray(gains, dtype=np.float32)
        b = np.ascontiguousarray(buses, dtype=np.uint8)
        assert g.size == self.shard_voices and b.size == self.shard_voices
        self._check(self.L.s2r_set_voice_mix(self.h, g.ctypes.data_as(_f32p), b.ctypes.data_as(C.POINTER(C.c_uint8))))

    def sample_buses(self, frames, sample_rate=SampleRateKhz(48000), n_buses=1):
        """the panned mixdown onto n_buses stereo buses from one render pass: (n_buses, frames, 2) float32"""
        out = np.empty(2 * frames * max(int(n_buses), 0), dtype=np.float32)
        self._check(self.L.s2r_fill_buses(self.h, out.ctypes.data_as(_f32p), out.size, int(n_buses), frames, int(sample_rate)))
        return out.reshape(n_buses, frames, 2)

    # --- live program faders (build-defined; s2r.h: s2r_set_program_fader) ---
    def set_program_fader(self, program, fader=1.0, pan_shift=0.0):
        """the target of a bank program's fader (in [0, 1]) and pan shift (in [-2, 2]): every voice sounding on the program
        reaches it as a ramp across the next sample_buses call.  Only sample_buses applies them."""
        self._check(self.L.s2r_set_program_fader(self.h, int(program), float(fader), float(pan_shift)))

    def get_program_fader(self, program):
        """(fader, pan_shift, applied_fader, applied_pan_shift): the target, and where the last bus fill left the pair"""
        f, sh, af, ash = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.s2r_get_program_fader(self.h, int(program), C.byref(f), C.byref(sh), C.byref(af), C.byref(ash)))
        return f.value, sh.value, af.value, ash.value

    def snap_program_faders(self):
        """applied = target for every program, now (a hard cut; restoring a checkpoint: set the applied values, snap, set the targets)"""
        self._check(self.L.s2r_snap_program_faders(self.h))

    # --- aux sends (build-defined; s2r.h: s2r_set_program_send) ---
    def set_program_send(self, program, send=0.0, send_bus=0):
        """the aux send (in [0, 1]) and the bus it feeds (below MAX_BUSES) of a bank program: what a note_on under that program
        gives its voice — a second feed of gain * send, post-pan and post-fader, onto send_bus.  Only sample_buses applies them."""
        self._check(self.L.s2r_set_program_send(self.h, int(program), float(send), int(send_bus)))

    def get_program_send(self, program):
        send, bus = C.c_float(), C.c_uint32()
        self._check(self.L.s2r_get_program_send(self.h, int(program), C.byref(send), C.byref(bus)))
        return send.value, bus.value

    def voice_sends(self):
        """(sends float32, send buses uint8) of every shard voice, local order (checkpoint companions of voice_mix)"""
        sends = np.empty(self.shard_voices, dtype=np.float32)
        buses = np.empty(self.shard_voices, dtype=np.uint8)
        self._check(self.L.s2r_get_voice_sends(self.h, sends.ctypes.data_as(_f32p), buses.ctypes.data_as(C.POINTER(C.c_uint8))))
        return sends, buses

    def set_voice_sends(self, sends, send_buses):
        g = np.ascontiguousarray(sends, dtype=np.float32)
        b = np.ascontiguousarray(send_buses, dtype=np.uint8)
        assert g.size == self.shard_voices and b.size == self.shard_voices
        self._check(self.L.s2r_set_voice_sends(self.h, g.ctypes.data_as(_f32p), b.ctypes.data_as(C.POINTER(C.c_uint8))))

    @staticmethod
    def send_gain(g, send):
        return send_gain(g, send)

    # --- per-bus convolution reverb (build-defined; s2r.h: s2r_set_bus_reverb) ---
    def set_bus_reverb(self, bus, ir, dry=0.0, wet=1.0):
        """a convolution reverb on a bus of sample_buses: ir is [K] (the same response for both channels) or [K, 2] (left, right),
        float32, 1 <= K <= MAX_IR_TAPS; dry and wet in [0, 1].  Replaces any earlier reverb of the bus and zeroes its history.  Only
        sample_buses applies it."""
        h = np.asarray(ir, dtype=np.float32)
        if h.ndim == 1:
            left = right = np.ascontiguousarray(h)
        elif h.ndim == 2 and h.shape[1] == 2:
            left, right = np.ascontiguousarray(h[:, 0]), np.ascontiguousarray(h[:, 1])
        else:
            raise ValueError("set_bus_reverb: ir is [K] or [K, 2]")
        if left.size < 1:
            raise ValueError("set_bus_reverb: at least one tap (clear_bus_reverb removes a reverb)")
        self._check(self.L.s2r_set_bus_reverb(self.h, int(bus), left.ctypes.data_as(_f32p), right.ctypes.data_as(_f32p), left.size, float(dry), float(wet)))

    def clear_bus_reverb(self, bus):
        """removes the bus's reverb: the bus returns the dry signal again, bit for bit"""
        self._check(self.L.s2r_set_bus_reverb(self.h, int(bus), None, None, 0, 0.0, 0.0))

    def set_bus_reverb_mix(self, bus, dry, wet):
        """dry and wet of the bus's reverb alone; taps and history stay"""
        self._check(self.L.s2r_set_bus_reverb_mix(self.h, int(bus), float(dry), float(wet)))

    def get_bus_reverb(self, bus):
        """(n_taps, dry, wet); n_taps is 0 for a bus without a reverb"""
        k, d, w = C.c_uint32(), C.c_float(), C.c_float()
        self._check(self.L.s2r_get_bus_reverb(self.h, int(bus), C.byref(k), C.byref(d), C.byref(w)))
        return k.value, d.value, w.value

    def bus_reverb_history(self, bus):
        """the K - 1 stereo frames the bus's reverb carries into the next sample_buses call, oldest first: (K - 1, 2) float32
        (the checkpoint companion of voice_sends)"""
        k = self.get_bus_reverb(bus)[0]
        out = np.empty((max(k, 1) - 1, 2), dtype=np.float32)
        self._check(self.L.s2r_get_bus_reverb_history(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out

    def set_bus_reverb_history(self, bus, history):
        h = np.ascontiguousarray(history, dtype=np.float32)
        if h.ndim != 2 or h.shape[1] != 2:
            raise ValueError("set_bus_reverb_history: history is [K - 1, 2]")
        self._check(self.L.s2r_set_bus_reverb_history(self.h, int(bus), h.ctypes.data_as(_f32p), h.size))

    @staticmethod
    def reverb_reference(ir, x_with_history, frames, dry, wet):
        return reverb_reference(ir, x_with_history, frames, dry, wet)

    # --- per-bus feedback delay (build-defined; s2r.h: s2r_set_bus_delay) ---
    def set_bus_delay(self, bus, delay_frames, feedback=0.0, cross=0.0, dry=1.0, wet=1.0):
        """a feedback delay of delay_frames (1 .. MAX_DELAY_FRAMES) on a bus of sample_buses and sample_master, in front of the bus's
        reverb: feedback and cross (the other channel's feed: ping-pong) in [-1, 1] with |feedback| + |cross| <= 1, dry and wet in
        [0, 1].  Replaces any earlier delay of the bus and zeroes its history."""
        if int(delay_frames) < 1:
            raise ValueError("set_bus_delay: at least one frame (clear_bus_delay removes a delay)")
        self._check(self.L.s2r_set_bus_delay(self.h, int(bus), int(delay_frames), float(feedback), float(cross), float(dry), float(wet)))

    def clear_bus_delay(self, bus):
        """removes the bus's delay: the bus returns the combine's signal again, bit for bit"""
        self._check(self.L.s2r_set_bus_delay(self.h, int(bus), 0, 0.0, 0.0, 0.0, 0.0))

    def set_bus_delay_mix(self, bus, feedback, cross, dry, wet):
        """the four levels of the bus's delay alone; its time and history stay"""
        self._check(self.L.s2r_set_bus_delay_mix(self.h, int(bus), float(feedback), float(cross), float(dry), float(wet)))

    def get_bus_delay(self, bus):
        """(delay_frames, feedback, cross, dry, wet); delay_frames is 0 for a bus without a delay"""
        n, f, x, d, w = C.c_uint32(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.s2r_get_bus_delay(self.h, int(bus), C.byref(n), C.byref(f), C.byref(x), C.byref(d), C.byref(w)))
        return n.value, f.value, x.value, d.value, w.value

    def bus_delay_history(self, bus):
        """the D stereo frames of the line that the bus's delay carries into the next call, oldest first: (D, 2) float32 (the
        checkpoint companion of bus_reverb_history)"""
        out = np.empty((self.get_bus_delay(bus)[0], 2), dtype=np.float32)
        self._check(self.L.s2r_get_bus_delay_history(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out

    def set_bus_delay_history(self, bus, history):
        h = np.ascontiguousarray(history, dtype=np.float32)
        if h.ndim != 2 or h.shape[1] != 2:
            raise ValueError("set_bus_delay_history: history is [D, 2]")
        self._check(self.L.s2r_set_bus_delay_history(self.h, int(bus), h.ctypes.data_as(_f32p), h.size))

    @staticmethod
    def delay_reference(delay_frames, feedback, cross, dry, wet, x, history):
        return delay_reference(delay_frames, feedback, cross, dry, wet, x, history)

    # --- per-bus chorus (build-defined; s2r.h: s2r_set_bus_chorus) ---
    def set_bus_chorus(self, bus, voices, base, depth, phase_inc, spread=0, dry=1.0, wet=1.0):
        """a chorus of `voices` (1 .. CHORUS_MAX_VOICES) taps on a bus of sample_buses and sample_master, in front of the bus's delay:
        each tap base + depth * triangle frames late (base >= 1, depth >= 0, float32(base + depth) <= CHORUS_MAX_DELAY), the LFO
        stepping phase_inc per frame (chorus_rate(hz, sample_rate)), the right channel `spread` ahead of the left, both in 2^-32 turns;
        dry and wet in [0, 1] (1 / voices goes into wet).  Replaces any earlier chorus of the bus and zeroes its history and phase."""
        if int(voices) < 1:
            raise ValueError("set_bus_chorus: at least one voice (clear_bus_chorus removes a chorus)")
        self._check(self.L.s2r_set_bus_chorus(self.h, int(bus), int(voices), float(base), float(depth), int(phase_inc) & 0xFFFFFFFF,
                                              int(spread) & 0xFFFFFFFF, float(dry), float(wet)))

    def clear_bus_chorus(self, bus):
        """removes the bus's chorus: the bus returns the combine's signal again, bit for bit"""
        self._check(self.L.s2r_set_bus_chorus(self.h, int(bus), 0, 0.0, 0.0, 0, 0, 0.0, 0.0))

    def set_bus_chorus_mix(self, bus, dry, wet):
        """the two levels of the bus's chorus alone; its state stays"""
        self._check(self.L.s2r_set_bus_chorus_mix(self.h, int(bus), float(dry), float(wet)))

    def set_bus_chorus_rate(self, bus, phase_inc, spread=0):
        """the LFO's step and the channels' spread alone; phase and history stay, so nothing clicks"""
        self._check(self.L.s2r_set_bus_chorus_rate(self.h, int(bus), int(phase_inc) & 0xFFFFFFFF, int(spread) & 0xFFFFFFFF))

    def get_bus_chorus(self, bus):
        """(voices, base, depth, phase_inc, spread, dry, wet); voices is 0 for a bus without a chorus"""
        v, pi, sp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        b, dp, d, w = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.s2r_get_bus_chorus(self.h, int(bus), C.byref(v), C.byref(b), C.byref(dp), C.byref(pi), C.byref(sp), C.byref(d), C.byref(w)))
        return v.value, b.value, dp.value, pi.value, sp.value, d.value, w.value

    def bus_chorus_state(self, bus):
        """what the bus's chorus carries into the next call: (the H stereo frames of its input's history, oldest first: (H, 2)
        float32, the LFO's phase) — the checkpoint companion of bus_delay_history"""
        _, base, depth = self.get_bus_chorus(bus)[:3]
        out = np.empty((chorus_history_frames(base, depth), 2), dtype=np.float32)
        ph = C.c_uint32()
        self._check(self.L.s2r_get_bus_chorus_state(self.h, int(bus), out.ctypes.data_as(_f32p), out.size, C.byref(ph)))
        return out, ph.value

    def set_bus_chorus_state(self, bus, history, phase):
        h = np.ascontiguousarray(history, dtype=np.float32)
        if h.ndim != 2 or h.shape[1] != 2:
            raise ValueError("set_bus_chorus_state: history is [H, 2]")
        self._check(self.L.s2r_set_bus_chorus_state(self.h, int(bus), h.ctypes.data_as(_f32p), h.size, int(phase) & 0xFFFFFFFF))

    @staticmethod
    def chorus_reference(voices, base, depth, phase_inc, spread, dry, wet, x, history, phase):
        return chorus_reference(voices, base, depth, phase_inc, spread, dry, wet, x, history, phase)

    @staticmethod
    def chorus_history_frames(base, depth):
        return chorus_history_frames(base, depth)

    @staticmethod
    def chorus_rate(hz, sample_rate):
        return chorus_rate(hz, sample_rate)

    # --- per-bus parametric EQ (build-defined; s2r.h: s2r_set_bus_eq) ---
    def set_bus_eq(self, bus, coeffs):
        """an EQ of 1 .. EQ_MAX_BANDS biquad bands on a bus of sample_buses and sample_master, at the head of the chain: coeffs
        [n_bands, 5] as (b0, b1, b2, a1, a2) per band (eq_design makes one), normalised by a0, finite, |a2| < 1 and |a1| < 1 + a2.
        Replaces any earlier EQ of the bus and zeroes its state."""
        c = _eq_coeffs(coeffs, "set_bus_eq")
        self._check(self.L.s2r_set_bus_eq(self.h, int(bus), c.shape[0], c.ctypes.data_as(_f32p)))

    def clear_bus_eq(self, bus):
        """removes the bus's EQ: the bus returns the combine's signal again, bit for bit"""
        self._check(self.L.s2r_set_bus_eq(self.h, int(bus), 0, None))

    def set_bus_eq_coeffs(self, bus, coeffs):
        """the coefficients of the bus's EQ alone, as many bands as it has; its state stays, so a band moves without a restart"""
        c = _eq_coeffs(coeffs, "set_bus_eq_coeffs")
        self._check(self.L.s2r_set_bus_eq_coeffs(self.h, int(bus), c.shape[0], c.ctypes.data_as(_f32p)))

    def get_bus_eq(self, bus):
        """the coefficients [n_bands, 5] float32 of the bus's EQ; [0, 5] for a bus without one"""
        n = C.c_uint32()
        out = np.empty((EQ_MAX_BANDS, 5), dtype=np.float32)
        self._check(self.L.s2r_get_bus_eq(self.h, int(bus), C.byref(n), out.ctypes.data_as(_f32p), out.size))
        return out[:n.value].copy()

    def bus_eq_state(self, bus):
        """what the bus's EQ carries into the next call: [n_bands, 4] float32 as (s1_L, s1_R, s2_L, s2_R) per band — the checkpoint
        companion of bus_chorus_state"""
        out = np.empty((self.get_bus_eq(bus).shape[0], 4), dtype=np.float32)
        self._check(self.L.s2r_get_bus_eq_state(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out

    def set_bus_eq_state(self, bus, state):
        st = np.ascontiguousarray(state, dtype=np.float32)
        if st.ndim != 2 or st.shape[1] != 4:
            raise ValueError("set_bus_eq_state: state is [n_bands, 4]")
        self._check(self.L.s2r_set_bus_eq_state(self.h, int(bus), st.ctypes.data_as(_f32p), st.size))

    @staticmethod
    def eq_reference(coeffs, x, state):
        return eq_reference(coeffs, x, state)

    @staticmethod
    def eq_design(kind, freq_hz, gain_db, q, sample_rate):
        return eq_design(kind, freq_hz, gain_db, q, sample_rate)

    # --- per-bus dynamics (build-defined; s2r.h: s2r_set_bus_dynamics) ---
    def set_bus_dynamics(self, bus, key_bus, curve, a_att, a_rel):
        """a sidechain compressor on a bus of sample_buses and sample_master, behind its EQ: key_bus == bus is the ordinary compressor,
        another bus a ducker; curve [DYN_CURVE_POINTS] float32 gains in [0, 256] (dynamics_curve makes one), a_att and a_rel in [0, 1)
        (dynamics_coef).  Replaces any earlier dynamics of the bus and resets the gain to curve[0]."""
        c = _dyn_curve(curve, "set_bus_dynamics")
        self._check(self.L.s2r_set_bus_dynamics(self.h, int(bus), int(key_bus), c.ctypes.data_as(_f32p), float(np.float32(a_att)), float(np.float32(a_rel))))

    def clear_bus_dynamics(self, bus):
        """removes the bus's dynamics: the bus passes again, bit for bit"""
        self._check(self.L.s2r_clear_bus_dynamics(self.h, int(bus)))

    def set_bus_dynamics_params(self, bus, key_bus, curve, a_att, a_rel):
        """key, curve and coefficients alone; the gain stays, so a threshold moves between calls without a restart"""
        c = _dyn_curve(curve, "set_bus_dynamics_params")
        self._check(self.L.s2r_set_bus_dynamics_params(self.h, int(bus), int(key_bus), c.ctypes.data_as(_f32p), float(np.float32(a_att)),
                                                       float(np.float32(a_rel))))

    def get_bus_dynamics(self, bus):
        """(key_bus, curve [DYN_CURVE_POINTS] float32, a_att, a_rel) of the bus's dynamics; None for a bus without"""
        present, key = C.c_uint32(), C.c_uint32()
        curve = np.empty(DYN_CURVE_POINTS, dtype=np.float32)
        a = np.empty(2, dtype=np.float32)
        self._check(self.L.s2r_get_bus_dynamics(self.h, int(bus), C.byref(present), C.byref(key), curve.ctypes.data_as(_f32p), curve.size,
                                                a[0:].ctypes.data_as(_f32p), a[1:].ctypes.data_as(_f32p)))
        return (key.value, curve, a[0], a[1]) if present.value else None

    def bus_dynamics_state(self, bus):
        """the gain the bus's dynamics carry into the next call, np.float32 — the checkpoint companion of bus_eq_state"""
        out = np.empty(1, dtype=np.float32)
        self._check(self.L.s2r_get_bus_dynamics_state(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out[0]

    def set_bus_dynamics_state(self, bus, y):
        st = np.array([y], dtype=np.float32)
        self._check(self.L.s2r_set_bus_dynamics_state(self.h, int(bus), st.ctypes.data_as(_f32p), st.size))

    def bus_dynamics_meter(self, bus):
        """the least gain of the last sample_buses / sample_master call that ran the bus's dynamics: 1.0 before any"""
        out = np.empty(1, dtype=np.float32)
        self._check(self.L.s2r_get_bus_dynamics_meter(self.h, int(bus), out.ctypes.data_as(_f32p)))
        return out[0]

    @staticmethod
    def dynamics_reference(curve, a_att, a_rel, key, x, y):
        return dynamics_reference(curve, a_att, a_rel, key, x, y)

    @staticmethod
    def dynamics_curve(threshold_db, ratio, knee_db=0.0, makeup_db=0.0):
        return dynamics_curve(threshold_db, ratio, knee_db, makeup_db)

    @staticmethod
    def dynamics_coef(ms, sample_rate):
        return dynamics_coef(ms, sample_rate)

    # --- per-bus room reverb (build-defined; s2r.h: s2r_set_bus_room) ---
    def set_bus_room(self, bus, cd, ad, spread, feedback, damp, g=0.5, gain=0.015, dry=1.0, wet=1.0, cross=0.0):
        """an algorithmic reverb on a bus of sample_buses and sample_master, the last stem writer: eight damped feedback combs cd [8]
        and four allpasses ad [4] per channel, delays in frames in [ROOM_MIN_DELAY, ROOM_MAX_DELAY], the right channel's `spread`
        frames longer (room_design makes a set); feedback in [0, 1), damp in [0, 1], g in (-1, 1), the others in [0, 1].  Replaces any
        earlier room of the bus and zeroes its state."""
        c, a = _room_delays(cd, ad, "set_bus_room")
        self._check(self.L.s2r_set_bus_room(self.h, int(bus), c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), int(spread),
                                            *_room_levels(feedback, damp, g, gain, dry, wet, cross)))

    def clear_bus_room(self, bus):
        """removes the bus's room: the bus passes again, bit for bit"""
        self._check(self.L.s2r_clear_bus_room(self.h, int(bus)))

    def set_bus_room_params(self, bus, feedback, damp, g, gain, dry, wet, cross):
        """the seven levels alone; delays and state stay, so room size and damping move between calls with no restart"""
        self._check(self.L.s2r_set_bus_room_params(self.h, int(bus), *_room_levels(feedback, damp, g, gain, dry, wet, cross)))

    def get_bus_room(self, bus):
        """(cd [8] uint32, ad [4] uint32, spread, feedback, damp, g, gain, dry, wet, cross) of the bus's room; None for a bus without"""
        present, sp = C.c_uint32(), C.c_uint32()
        c = np.empty(ROOM_COMBS, dtype=np.uint32)
        a = np.empty(ROOM_ALLPASSES, dtype=np.uint32)
        lv = np.empty(7, dtype=np.float32)
        self._check(self.L.s2r_get_bus_room(self.h, int(bus), C.byref(present), c.ctypes.data_as(_u32p), a.ctypes.data_as(_u32p), C.byref(sp),
                                            lv.ctypes.data_as(_f32p)))
        return (c, a, sp.value) + tuple(lv) if present.value else None

    def bus_room_state(self, bus):
        """the state the bus's room carries into the next call, flat float32 (s2r.h gives the layout) — the checkpoint companion of
        bus_eq_state"""
        r = self.get_bus_room(bus)
        n = room_state_floats(r[0], r[1], r[2]) if r else 1
        out = np.empty(n, dtype=np.float32)
        self._check(self.L.s2r_get_bus_room_state(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out

    def set_bus_room_state(self, bus, state):
        st = np.ascontiguousarray(state, dtype=np.float32).ravel()
        self._check(self.L.s2r_set_bus_room_state(self.h, int(bus), st.ctypes.data_as(_f32p), st.size))

    @staticmethod
    def room_reference(cd, ad, spread, feedback, damp, g, gain, dry, wet, cross, x, state=None):
        return room_reference(cd, ad, spread, feedback, damp, g, gain, dry, wet, cross, x, state)

    @staticmethod
    def room_design(sample_rate, size=1.0):
        return room_design(sample_rate, size)

    # --- per-bus drive (build-defined; s2r.h: s2r_set_bus_drive) ---
    def set_bus_drive(self, bus, curve, pre=1.0, dry=0.0, wet=1.0):
        """an oversampled waveshaper on a bus of sample_buses and sample_master, behind the dynamics: curve [DRIVE_CURVE_POINTS] float32,
        finite, entry 512 its value at 0 and entry 512 +- i at +- i / 512 (drive_curve makes one); pre in [0, DRIVE_MAX_PRE], dry and
        wet in [0, 1].  The bus comes out DRIVE_LATENCY frames late.  Replaces any earlier drive of the bus and zeroes its history."""
        c = _drive_curve(curve, "set_bus_drive")
        self._check(self.L.s2r_set_bus_drive(self.h, int(bus), c.ctypes.data_as(_f32p), _f32(pre), _f32(dry), _f32(wet)))

    def clear_bus_drive(self, bus):
        """removes the bus's drive: the bus passes again, bit for bit"""
        self._check(self.L.s2r_clear_bus_drive(self.h, int(bus)))

    def set_bus_drive_params(self, bus, curve, pre, dry, wet):
        """the levels, and the table unless curve is None; the history stays, so a curve or a level moves between calls with no restart"""
        c = None if curve is None else _drive_curve(curve, "set_bus_drive_params")
        self._check(self.L.s2r_set_bus_drive_params(self.h, int(bus), None if c is None else c.ctypes.data_as(_f32p), _f32(pre), _f32(dry), _f32(wet)))

    def get_bus_drive(self, bus):
        """(curve [DRIVE_CURVE_POINTS] float32, pre, dry, wet) of the bus's drive; None for a bus without"""
        present = C.c_uint32()
        curve = np.empty(DRIVE_CURVE_POINTS, dtype=np.float32)
        pre, dry, wet = C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.s2r_get_bus_drive(self.h, int(bus), C.byref(present), curve.ctypes.data_as(_f32p), curve.size, C.byref(pre), C.byref(dry),
                                             C.byref(wet)))
        return (curve, np.float32(pre.value), np.float32(dry.value), np.float32(wet.value)) if present.value else None

    def bus_drive_history(self, bus):
        """the [DRIVE_HISTORY, 2] float32 input frames the bus's drive carries into the next call, oldest first — the checkpoint
        companion of bus_delay_history"""
        out = np.empty((DRIVE_HISTORY, 2), dtype=np.float32)
        self._check(self.L.s2r_get_bus_drive_history(self.h, int(bus), out.ctypes.data_as(_f32p), out.size))
        return out

    def set_bus_drive_history(self, bus, history):
        st = np.ascontiguousarray(history, dtype=np.float32).ravel()
        self._check(self.L.s2r_set_bus_drive_history(self.h, int(bus), st.ctypes.data_as(_f32p), st.size))

    @staticmethod
    def drive_reference(curve, pre, dry, wet, x, history=None):
        return drive_reference(curve, pre, dry, wet, x, history)

    @staticmethod
    def drive_curve(kind, amount=1.0):
        return drive_curve(kind, amount)

    @staticmethod
    def drive_taps():
        return drive_taps()

    # --- per-bus flanger (build-defined; s2r.h: s2r_set_bus_flanger) ---
    def set_bus_flanger(self, bus, base, depth, phase_inc, spread=0, feedback=0.0, cross=0.0, dry=1.0, wet=1.0):
        """a flanger on a bus of sample_buses and sample_master, behind the drive and in front of the chorus: one tap base + depth *
        triangle frames late (base >= FLANGER_MIN_DELAY, depth >= 0, float32(base + depth) <= FLANGER_MAX_DELAY) into the stage's own line
        signal, fed back by `feedback` and into the other channel by `cross` (each in [-1, 1], |feedback| + |cross| <= 1); the LFO steps
        phase_inc per frame (chorus_rate(hz, sample_rate)), the right channel `spread` ahead of the left, both in 2^-32 turns; dry and
        wet in [0, 1].  Replaces any earlier flanger of the bus and zeroes its history and phase."""
        self._check(self.L.s2r_set_bus_flanger(self.h, int(bus), float(base), float(depth), int(phase_inc) & 0xFFFFFFFF, int(spread) & 0xFFFFFFFF,
                                               float(feedback), float(cross), float(dry), float(wet)))

    def clear_bus_flanger(self, bus):
        """removes the bus's flanger: the bus passes again, bit for bit"""
        self._check(self.L.s2r_clear_bus_flanger(self.h, int(bus)))

    def set_bus_flanger_params(self, bus, phase_inc, spread, feedback, cross, dry, wet):
        """everything but base and depth; history and phase stay, so rate and resonance move between calls without a click"""
        self._check(self.L.s2r_set_bus_flanger_params(self.h, int(bus), int(phase_inc) & 0xFFFFFFFF, int(spread) & 0xFFFFFFFF, float(feedback), float(cross),
                                                      float(dry), float(wet)))

    def get_bus_flanger(self, bus):
        """(base, depth, phase_inc, spread, feedback, cross, dry, wet); base is 0 for a bus without a flanger"""
        b, dp, fb, cr, d, w = (C.c_float() for _ in range(6))
        pi, sp = C.c_uint32(), C.c_uint32()
        self._check(self.L.s2r_get_bus_flanger(self.h, int(bus), C.byref(b), C.byref(dp), C.byref(pi), C.byref(sp), C.byref(fb), C.byref(cr), C.byref(d),
                                               C.byref(w)))
        return (np.float32(b.value), np.float32(dp.value), pi.value, sp.value, np.float32(fb.value), np.float32(cr.value), np.float32(d.value),
                np.float32(w.value))

    def bus_flanger_state(self, bus):
        """what the bus's flanger carries into the next call: (the H stereo frames of its line signal, oldest first: (H, 2) float32, the
        LFO's phase) — the checkpoint companion of bus_chorus_state"""
        base, depth = self.get_bus_flanger(bus)[:2]
        out = np.empty((flanger_history_frames(base, depth), 2), dtype=np.float32)
        ph = C.c_uint32()
        self._check(self.L.s2r_get_bus_flanger_state(self.h, int(bus), out.ctypes.data_as(_f32p), out.size, C.byref(ph)))
        return out, ph.value

    def set_bus_flanger_state(self, bus, history, phase):
        h = np.ascontiguousarray(history, dtype=np.float32)
        if h.ndim != 2 or h.shape[1] != 2:
            raise ValueError("set_bus_flanger_state: history is [H, 2]")
        self._check(self.L.s2r_set_bus_flanger_state(self.h, int(bus), h.ctypes.data_as(_f32p), h.size, int(phase) & 0xFFFFFFFF))

    @staticmethod
    def flanger_reference(base, depth, phase_inc, spread, feedback, cross, dry, wet, x, history, phase):
        return flanger_reference(base, depth, phase_inc, spread, feedback, cross, dry, wet, x, history, phase)

    @staticmethod
    def flanger_history_frames(base, depth):
        return flanger_history_frames(base, depth)

    # --- the master section (build-defined; s2r.h: s2r_fill_master) ---
    def set_bus_return(self, bus, level=1.0):
        """the target of a bus's return level (in [0, 1]): reached as a ramp across the next sample_master call.  Only sample_master
        applies returns, the master fader and the meters."""
        self._check(self.L.s2r_set_bus_return(self.h, int(bus), float(level)))

    def get_bus_return(self, bus):
        """(level, applied): the target, and where the last master fill left the return"""
        t, a = C.c_float(), C.c_float()
        self._check(self.L.s2r_get_bus_return(self.h, int(bus), C.byref(t), C.byref(a)))
        return t.value, a.value

    def set_master_fader(self, level=1.0):
        self._check(self.L.s2r_set_master_fader(self.h, float(level)))

    def get_master_fader(self):
        """(level, applied)"""
        t, a = C.c_float(), C.c_float()
        self._check(self.L.s2r_get_master_fader(self.h, C.byref(t), C.byref(a)))
        return t.value, a.value

    def snap_master(self):
        """applied = target for every return and the master fader, now (a hard cut; restoring a checkpoint: set the applied values,
        snap, set the targets)"""
        self._check(self.L.s2r_snap_master(self.h))

    def sample_master(self, frames, sample_rate=SampleRateKhz(48000), n_buses=1, stems=True):
        """sample_buses with the master section behind it: (master [frames, 2], stems [n_buses, frames, 2]), or (master, None) with
        stems=False — the stems then never cross to the host"""
        out = np.empty(2 * frames, dtype=np.float32)
        st = np.empty(2 * frames * max(int(n_buses), 0), dtype=np.float32) if stems else None
        self._check(self.L.s2r_fill_master(self.h, out.ctypes.data_as(_f32p), st.ctypes.data_as(_f32p) if stems else None,
                                           st.size if stems else 0, int(n_buses), frames, int(sample_rate)))
        return out.reshape(frames, 2), (st.reshape(n_buses, frames, 2) if stems else None)

    def meters(self):
        """(peak, energy) of the last successful sample_master call, each [n_buses + 1, 2] float32: the buses (post-effect,
        pre-return), then the master"""
        n = C.c_uint32()
        peak = np.empty(2 * (MAX_BUSES + 1), dtype=np.float32)
        energy = np.empty(2 * (MAX_BUSES + 1), dtype=np.float32)
        self._check(self.L.s2r_get_meters(self.h, C.byref(n), peak.ctypes.data_as(_f32p), energy.ctypes.data_as(_f32p), peak.size))
        k = 2 * (n.value + 1)
        return peak[:k].reshape(-1, 2).copy(), energy[:k].reshape(-1, 2).copy()

    @staticmethod
    def master_reference(stems, r0, r1, m0, m1):
        return master_reference(stems, r0, r1, m0, m1)

    # --- the master limiter (build-defined; s2r.h: s2r_set_master_limiter) ---
    def set_master_limiter(self, ceiling, lookahead, hold=0, true_peak=False):
        """a look-ahead limiter behind the master fader, in sample_master only: no sample of the master exceeds `ceiling`, and the
        master is delayed by `lookahead` frames (the stems are not).  true_peak: the gain follows the 4x-interpolated magnitude of the
        master, not its samples' (s2r.h: s2r_set_master_limiter_ex), and the delay is LIMITER_TP_LATENCY frames longer.  A new
        lookahead, hold or detector resets the state; a new ceiling alone keeps it."""
        if true_peak:
            self._check(self.L.s2r_set_master_limiter_ex(self.h, float(ceiling), int(lookahead), int(hold), LIMITER_TRUE_PEAK))
        else:
            self._check(self.L.s2r_set_master_limiter(self.h, float(ceiling), int(lookahead), int(hold)))

    def clear_master_limiter(self):
        self._check(self.L.s2r_clear_master_limiter(self.h))

    def get_master_limiter(self):
        """(ceiling, lookahead, hold); a lookahead of 0 means off"""
        c, l, h = C.c_float(), C.c_uint32(), C.c_uint32()
        self._check(self.L.s2r_get_master_limiter(self.h, C.byref(c), C.byref(l), C.byref(h)))
        return c.value, l.value, h.value

    def get_master_limiter_detector(self):
        """LIMITER_SAMPLE_PEAK or LIMITER_TRUE_PEAK; 0 with the limiter off"""
        d = C.c_uint32()
        self._check(self.L.s2r_get_master_limiter_detector(self.h, C.byref(d)))
        return d.value

    def limiter_state(self):
        """(xh [lookahead, 2], gh [2 * lookahead + hold]): the limiter's carried input frames and gains, oldest first (checkpoints);
        xh is [lookahead + LIMITER_TP_HISTORY, 2] with the true-peak detector"""
        _, l, h = self.get_master_limiter()
        more = LIMITER_TP_HISTORY if self.get_master_limiter_detector() == LIMITER_TRUE_PEAK else 0
        xh, gh = np.empty((l + more, 2), dtype=np.float32), np.empty(2 * l + h, dtype=np.float32)
        self._check(self.L.s2r_get_limiter_state(self.h, xh.ctypes.data_as(_f32p), xh.size, gh.ctypes.data_as(_f32p), gh.size))
        return xh, gh

    def set_limiter_state(self, xh, gh):
        xh = np.ascontiguousarray(xh, dtype=np.float32)
        gh = np.ascontiguousarray(gh, dtype=np.float32)
        self._check(self.L.s2r_set_limiter_state(self.h, xh.ctypes.data_as(_f32p), xh.size, gh.ctypes.data_as(_f32p), gh.size))

    def limiter_meters(self):
        """(min_gain, out_peak) of the last successful sample_master call that ran the limiter"""
        g, p = C.c_float(), C.c_float()
        self._check(self.L.s2r_get_limiter_meters(self.h, C.byref(g), C.byref(p)))
        return g.value, p.value

    @staticmethod
    def limiter_reference(x, ceiling, lookahead, hold, xh=None, gh=None):
        return limiter_reference(x, ceiling, lookahead, hold, xh, gh)

    @staticmethod
    def limiter_tp_reference(x, ceiling, lookahead, hold, xh=None, gh=None):
        return limiter_tp_reference(x, ceiling, lookahead, hold, xh, gh)

    # --- the loudness and true-peak meters (build-defined; s2r.h: s2r_set_master_loudness) ---
    def set_master_loudness(self, sample_rate=48000, hop=None, max_hops=None, coeffs=None):
        """BS.1770 loudness meters on every bus and the master, and the master's true peak, behind the limiter, in sample_master only.
        `hop`: the frames of 100 ms (None: sample_rate / 10); `max_hops`: the hop rows kept for the integrated value (None: an hour's);
        `coeffs`: the two biquads [2, 5] (None: loudness_design(sample_rate)).  Starts from the initial state with no rows."""
        hop = int(round(float(sample_rate) / 10.0)) if hop is None else int(hop)
        max_hops = 36000 if max_hops is None else int(max_hops)
        c = loudness_design(sample_rate) if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.float32)
        if c.size != 10:
            raise ValueError("set_master_loudness: coeffs is [2, 5]")
        self._check(self.L.s2r_set_master_loudness(self.h, c.ctypes.data_as(_f32p), hop, max_hops))

    def clear_master_loudness(self):
        self._check(self.L.s2r_clear_master_loudness(self.h))

    def get_master_loudness(self):
        """(coeffs [2, 5], hop, max_hops, n_hops): a hop of 0 means off; n_hops the hop rows stored"""
        c, h, m, n = np.empty((2, 5), dtype=np.float32), C.c_uint32(), C.c_uint32(), C.c_size_t()
        self._check(self.L.s2r_get_master_loudness(self.h, c.ctypes.data_as(_f32p), C.byref(h), C.byref(m), C.byref(n)))
        return c, h.value, m.value, n.value

    def reset_master_loudness(self):
        """state, rows and the held true peak cleared; the parameters stay"""
        self._check(self.L.s2r_reset_master_loudness(self.h))

    def loudness(self, programme=MAX_BUSES):
        """(momentary, short-term, integrated) in LKFS of bus `programme`, or of the master (MAX_BUSES), over the stored hop rows"""
        out = (C.c_double * 3)()
        self._check(self.L.s2r_get_loudness(self.h, int(programme), out))
        return out[0], out[1], out[2]

    def true_peak(self):
        """(last [2], held [2]): the master's true peak, L and R, of the last sample_master call and since the last reset"""
        last, held = np.empty(2, dtype=np.float32), np.empty(2, dtype=np.float32)
        self._check(self.L.s2r_get_true_peak(self.h, last.ctypes.data_as(_f32p), held.ctypes.data_as(_f32p)))
        return last, held

    def loudness_state(self):
        """(state [LOUDNESS_STATE], pos): the filters' values, the partial hop sums, the master's last 16 frames; the frames of the hop
        under way (checkpoints)"""
        st, pos = np.empty(LOUDNESS_STATE, dtype=np.float32), C.c_uint32()
        self._check(self.L.s2r_get_loudness_state(self.h, st.ctypes.data_as(_f32p), st.size, C.byref(pos)))
        return st, pos.value

    def set_loudness_state(self, state, pos):
        st = np.ascontiguousarray(state, dtype=np.float32)
        self._check(self.L.s2r_set_loudness_state(self.h, st.ctypes.data_as(_f32p), st.size, int(pos)))

    def loudness_hops(self):
        """the stored hop rows, oldest first: [n_hops, 18] float32 (checkpoints)"""
        n = self.get_master_loudness()[3]
        rows, got = np.empty((n, LOUDNESS_CHANNELS), dtype=np.float32), C.c_size_t()
        self._check(self.L.s2r_get_loudness_hops(self.h, rows.ctypes.data_as(_f32p) if n else None, rows.size, C.byref(got)))
        return rows[:got.value]

    def set_loudness_hops(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = rows.shape[0] if rows.ndim == 2 else rows.size // LOUDNESS_CHANNELS
        self._check(self.L.s2r_set_loudness_hops(self.h, rows.ctypes.data_as(_f32p) if rows.size else None, n, rows.size))

    @staticmethod
    def loudness_reference(coeffs, hop, stems, master, state=None, pos=0):
        return loudness_reference(coeffs, hop, stems, master, state, pos)

    @staticmethod
    def loudness_readings(rows, hop, programme):
        return loudness_readings(rows, hop, programme)

    @staticmethod
    def loudness_design(sample_rate=48000.0):
        return loudness_design(sample_rate)

    # --- the spectrum meters (build-defined; s2r.h: s2r_set_master_spectrum) ---
    def set_master_spectrum(self, n_fft, hop, window="hann", max_rows=16):
        """a windowed power spectrum of every bus and the master, behind the loudness meters, in sample_master only.  `n_fft`: a power
        of two, 256 .. 8192; `hop`: frames between rows, at least n_fft / 8; `window`: a kind for spectrum_window or n_fft values;
        `max_rows`: the rows kept (1 .. 256).  Starts from the initial state with no rows."""
        w = _spectrum_window_arg(window, n_fft) if 0 < int(n_fft) <= (1 << 20) else np.zeros(1, dtype=np.float32)
        self._check(self.L.s2r_set_master_spectrum(self.h, int(n_fft), int(hop), w.ctypes.data_as(_f32p), int(max_rows)))

    def clear_master_spectrum(self):
        self._check(self.L.s2r_clear_master_spectrum(self.h))

    def get_master_spectrum(self):
        """(n_fft, hop, max_rows, n_rows, window [n_fft]): an n_fft of 0 means off; n_rows the rows stored"""
        n, h, m, k = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        self._check(self.L.s2r_get_master_spectrum(self.h, C.byref(n), C.byref(h), C.byref(m), C.byref(k), None, 0))
        w = np.empty(n.value, dtype=np.float32)
        if n.value:
            self._check(self.L.s2r_get_master_spectrum(self.h, None, None, None, None, w.ctypes.data_as(_f32p), w.size))
        return n.value, h.value, m.value, k.value, w

    def reset_master_spectrum(self):
        """state and rows cleared; the parameters stay"""
        self._check(self.L.s2r_reset_master_spectrum(self.h))

    def spectrum(self, programme=MAX_BUSES, n_avg=1):
        """dB per bin [n_fft / 2 + 1] of bus `programme`, or of the master (MAX_BUSES), over the last n_avg stored rows"""
        out = np.empty(self.get_master_spectrum()[0] // 2 + 1, dtype=np.float64)
        self._check(self.L.s2r_get_spectrum(self.h, int(programme), int(n_avg), out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def spectrum_bands(self, programme, sample_rate, bands_per_octave, n_avg=1):
        """(dB [n_bands], centres in Hz [n_bands]) per fractional-octave band over the last n_avg stored rows"""
        cap = 256
        db, fc, n = np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.float64), C.c_size_t(0)
        dp = C.POINTER(C.c_double)
        self._check(self.L.s2r_get_spectrum_bands(self.h, int(programme), int(n_avg), float(sample_rate), int(bands_per_octave), db.ctypes.data_as(dp),
                                                  fc.ctypes.data_as(dp), cap, C.byref(n)))
        return db[:n.value].copy(), fc[:n.value].copy()

    def spectrum_rows(self):
        """the stored rows, oldest first: [n_rows, 9, n_fft / 2 + 1] float32 (checkpoints)"""
        n_fft, _, _, n, _ = self.get_master_spectrum()
        rows, got = np.empty((n, SPECTRUM_PROGRAMMES, n_fft // 2 + 1), dtype=np.float32), C.c_size_t()
        self._check(self.L.s2r_get_spectrum_rows(self.h, rows.ctypes.data_as(_f32p) if n else None, rows.size, C.byref(got)))
        return rows[:got.value]

    def set_spectrum_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        self._check(self.L.s2r_set_spectrum_rows(self.h, rows.ctypes.data_as(_f32p) if rows.size else None, rows.shape[0] if rows.ndim == 3 else 0, rows.size))

    def spectrum_state(self):
        """(state [9, n_fft, 2], pos): the last n_fft frames of every programme, oldest first; the frames of the hop under way"""
        n_fft = self.get_master_spectrum()[0]
        st, pos = np.empty((SPECTRUM_PROGRAMMES, n_fft, 2), dtype=np.float32), C.c_uint32()
        self._check(self.L.s2r_get_spectrum_state(self.h, st.ctypes.data_as(_f32p), st.size, C.byref(pos)))
        return st, pos.value

    def set_spectrum_state(self, state, pos):
        st = np.ascontiguousarray(state, dtype=np.float32)
        self._check(self.L.s2r_set_spectrum_state(self.h, st.ctypes.data_as(_f32p), st.size, int(pos)))

    @staticmethod
    def spectrum_reference(n_fft, hop, window, stems, master, state=None, pos=0):
        return spectrum_reference(n_fft, hop, window, stems, master, state, pos)

    @staticmethod
    def spectrum_readings(rows, window, programme, n_avg=1):
        return spectrum_readings(rows, window, programme, n_avg)

    @staticmethod
    def spectrum_band_readings(rows, window, programme, sample_rate, bands_per_octave, n_avg=1):
        return spectrum_band_readings(rows, window, programme, sample_rate, bands_per_octave, n_avg)

    @staticmethod
    def spectrum_window(kind, n_fft):
        return spectrum_window(kind, n_fft)

    @staticmethod
    def spectrum_twiddles(n_fft):
        return spectrum_twiddles(n_fft)

    # --- the PCM stage (build-defined; s2r.h: s2r_set_master_pcm) ---
    def set_master_pcm(self, bits=16, dither="tpdf", shaper=0, seed=0):
        """integers of `bits` bits (8 .. 24) of every bus and the master, behind the spectrum meters, in sample_master only.  `dither`:
        'none', 'rect' or 'tpdf' (or a DITHER_* value); `shaper`: a SHAPER_* kind or up to nine error-feedback taps; `seed`: the
        dither's.  Starts from the initial state."""
        taps = _shaper_arg(shaper)
        self._check(self.L.s2r_set_master_pcm(self.h, int(bits), _dither_arg(dither), taps.ctypes.data_as(_f32p) if taps.size else None, taps.size,
                                              int(seed) & 0xffffffff))

    def clear_master_pcm(self):
        self._check(self.L.s2r_clear_master_pcm(self.h))

    def get_master_pcm(self):
        """(bits, dither, taps [n_taps], seed): bits of 0 means off"""
        b, d, n, sd = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        taps = np.empty(PCM_MAX_TAPS, dtype=np.float32)
        self._check(self.L.s2r_get_master_pcm(self.h, C.byref(b), C.byref(d), taps.ctypes.data_as(_f32p), C.byref(n), C.byref(sd)))
        return b.value, d.value, taps[:n.value].copy(), sd.value

    def reset_master_pcm(self):
        """state, frame count and clip counts cleared; the parameters stay"""
        self._check(self.L.s2r_reset_master_pcm(self.h))

    def pcm(self, programme=MAX_BUSES):
        """int32 [frames, 2]: the samples of bus `programme`, or of the master (MAX_BUSES), of the last sample_master call"""
        # Behind the resampler a call can make more frames than it was given, and the samples stay held when that resampler is
        # cleared or replaced by one of a smaller ratio: the buffer is sized by the largest ratio a resampler can have, 4, not by
        # the one that is set now
        most = resampler_max_out(self.max_frames, RESAMPLER_MAX_RATIO, 1)
        out, n = np.empty((most, 2), dtype=np.int32), C.c_size_t()
        self._check(self.L.s2r_get_pcm(self.h, int(programme), out.ctypes.data_as(C.POINTER(C.c_int32)), out.size, C.byref(n)))
        return out[:n.value].copy()

    def pcm_clips(self):
        """(last [18], held [18]) uint32: the clips per channel of the last sample_master call and since the set or reset"""
        last, held = np.empty(PCM_CHANNELS, dtype=np.uint32), np.empty(PCM_CHANNELS, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._check(self.L.s2r_get_pcm_clips(self.h, last.ctypes.data_as(u32p), held.ctypes.data_as(u32p)))
        return last, held

    def pcm_state(self):
        """(state [18, 9], t): every channel's last nine shaped errors, newest first; the frames converted (checkpoints)"""
        st, t = np.empty((PCM_CHANNELS, PCM_MAX_TAPS), dtype=np.float32), C.c_uint32()
        self._check(self.L.s2r_get_pcm_state(self.h, st.ctypes.data_as(_f32p), st.size, C.byref(t)))
        return st, t.value

    def set_pcm_state(self, state, t):
        st = np.ascontiguousarray(state, dtype=np.float32)
        self._check(self.L.s2r_set_pcm_state(self.h, st.ctypes.data_as(_f32p), st.size, int(t) & 0xffffffff))

    @staticmethod
    def pcm_reference(stems, master, bits=16, dither="tpdf", shaper=0, seed=0, state=None, t=0):
        return pcm_reference(stems, master, bits, dither, shaper, seed, state, t)

    @staticmethod
    def pcm_dither(seed, t, q, kind="tpdf"):
        return pcm_dither(seed, t, q, kind)

    @staticmethod
    def pcm_pack(pcm, bits, bytes_per_sample):
        return pcm_pack(pcm, bits, bytes_per_sample)

    @staticmethod
    def pcm_shaper(kind):
        return pcm_shaper(kind)

    # --- the sample-rate converter (build-defined; s2r.h: s2r_set_master_resampler) ---
    def set_master_resampler(self, L, M, table):
        """every bus and the master resampled by L / M through the polyphase table [L, T] (resampler_design makes one), behind the
        spectrum meters and in front of the PCM stage, in sample_master only.  Starts from the initial state."""
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.ndim != 2 or table.shape[0] != int(L):
            raise ValueError("set_master_resampler: table is [L, T]")
        self._check(self.L.s2r_set_master_resampler(self.h, int(L), int(M), table.shape[1], table.ctypes.data_as(_f32p)))

    def clear_master_resampler(self):
        self._check(self.L.s2r_clear_master_resampler(self.h))

    def get_master_resampler(self):
        """(L, M, table [L, T]): L of 0 means off (and the table is None)"""
        l, m, t = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.s2r_get_master_resampler(self.h, C.byref(l), C.byref(m), C.byref(t), None))
        if not l.value:
            return 0, 0, None
        table = np.empty((l.value, t.value), dtype=np.float32)
        self._check(self.L.s2r_get_master_resampler(self.h, None, None, None, table.ctypes.data_as(_f32p)))
        return l.value, m.value, table

    def reset_master_resampler(self):
        """history and position cleared; the parameters stay"""
        self._check(self.L.s2r_reset_master_resampler(self.h))

    def resampled(self, programme=MAX_BUSES):
        """float32 [count, 2]: the resampled frames of bus `programme`, or of the master (MAX_BUSES), of the last sample_master call"""
        l, m = C.c_uint32(), C.c_uint32()
        self._check(self.L.s2r_get_master_resampler(self.h, C.byref(l), C.byref(m), None, None))
        out, n = np.empty((resampler_max_out(self.max_frames, l.value, max(m.value, 1)), 2), dtype=np.float32), C.c_size_t()
        self._check(self.L.s2r_get_resampled(self.h, int(programme), out.ctypes.data_as(_f32p), out.size, C.byref(n)))
        return out[:n.value].copy()

    def resampler_state(self):
        """(state [18, T - 1], ph): every channel's last T - 1 input frames, newest first; the next output's position (checkpoints)"""
        t, ph = C.c_uint32(), C.c_uint32()
        self._check(self.L.s2r_get_master_resampler(self.h, None, None, C.byref(t), None))
        st = np.empty((RESAMPLER_CHANNELS, max(t.value, 1) - 1), dtype=np.float32)
        self._check(self.L.s2r_get_resampler_state(self.h, st.ctypes.data_as(_f32p), st.size, C.byref(ph)))
        return st, ph.value

    def set_resampler_state(self, state, ph):
        st = np.ascontiguousarray(state, dtype=np.float32)
        self._check(self.L.s2r_set_resampler_state(self.h, st.ctypes.data_as(_f32p), st.size, int(ph)))

    @staticmethod
    def resampler_reference(stems, master, L, M, table, state=None, ph=0):
        return resampler_reference(stems, master, L, M, table, state, ph)

    @staticmethod
    def resampler_count(L, M, ph, frames):
        return resampler_count(L, M, ph, frames)

    @staticmethod
    def resampler_design(L, M, T, beta=10.0, rolloff=0.9):
        return resampler_design(L, M, T, beta, rolloff)

    # --- the master multiband compressor (build-defined; s2r.h: s2r_set_master_multiband) ---
    def _multiband(self, who, entry, splits_hz, coeffs, curves, attack, release, sample_rate):
        if splits_hz is not None and coeffs is not None:
            raise ValueError(who + ": give splits_hz or coeffs, not both")
        if splits_hz is not None:
            coeffs = multiband_design(sample_rate, splits_hz)
        B, lp, hp, ap, cv, att, rel = _multiband_args(who, coeffs, curves, attack, release)
        self._check(entry(self.h, B, _f32_or_null(lp), _f32_or_null(hp), _f32_or_null(ap), cv.ctypes.data_as(_f32p), att.ctypes.data_as(_f32p),
                          rel.ctypes.data_as(_f32p)))

    def set_master_multiband(self, curves, attack, release, splits_hz=None, coeffs=None, sample_rate=48000.0):
        """the master split into len(curves) bands between the master fader and the limiter, each compressed by its own curve
        [DYN_CURVE_POINTS] and retention coefficients, and added back (s2r.h): splits_hz designs the crossover at `sample_rate`
        (multiband_design), or coeffs = (lp, hp, ap) gives its rows; one band needs neither.  The state starts afresh."""
        self._multiband("set_master_multiband", self.L.s2r_set_master_multiband, splits_hz, coeffs, curves, attack, release, sample_rate)

    def set_master_multiband_params(self, curves, attack, release, splits_hz=None, coeffs=None, sample_rate=48000.0):
        """the same arguments with the band count that is set: the parameters change, the state stays"""
        self._multiband("set_master_multiband_params", self.L.s2r_set_master_multiband_params, splits_hz, coeffs, curves, attack, release, sample_rate)

    def clear_master_multiband(self):
        self._check(self.L.s2r_clear_master_multiband(self.h))

    def _multiband_bands(self):
        b = C.c_uint32()
        self._check(self.L.s2r_get_master_multiband(self.h, C.byref(b), None, None, None, None, None, None))
        return b.value

    def get_master_multiband(self):
        """None when off, else dict(n_bands, lp, hp, ap, curves, attack, release)"""
        B = self._multiband_bands()
        if not B:
            return None
        lp, hp, ap = np.zeros((B - 1, 5), np.float32), np.zeros((B - 1, 5), np.float32), np.zeros((max(B - 2, 0), 5), np.float32)
        cv, att, rel = np.zeros((B, DYN_CURVE_POINTS), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        self._check(self.L.s2r_get_master_multiband(self.h, None, _f32_or_null(lp), _f32_or_null(hp), _f32_or_null(ap), cv.ctypes.data_as(_f32p),
                                                    att.ctypes.data_as(_f32p), rel.ctypes.data_as(_f32p)))
        return dict(n_bands=B, lp=lp, hp=hp, ap=ap, curves=cv, attack=att, release=rel)

    def reset_master_multiband(self):
        """filters and gains as right after a set; the parameters stay"""
        self._check(self.L.s2r_reset_master_multiband(self.h))

    def multiband_state(self):
        """float32 [multiband_state_floats(B)]: every section's (s1_L, s1_R, s2_L, s2_R), then the bands' gains (checkpoints)"""
        B = self._multiband_bands()
        st = np.empty(multiband_state_floats(B) if B else 1, dtype=np.float32)
        self._check(self.L.s2r_get_multiband_state(self.h, st.ctypes.data_as(_f32p), st.size))
        return st

    def set_multiband_state(self, state):
        st = np.ascontiguousarray(state, dtype=np.float32).reshape(-1)
        self._check(self.L.s2r_set_multiband_state(self.h, st.ctypes.data_as(_f32p), st.size))

    def multiband_meters(self):
        """float32 [B]: every band's minimum of y over the last sample_master call that ran the stage"""
        mn = np.empty(MULTIBAND_MAX_BANDS, dtype=np.float32)
        B = self._multiband_bands()
        self._check(self.L.s2r_get_multiband_meters(self.h, mn.ctypes.data_as(_f32p), mn.size))
        return mn[:B].copy()

    @staticmethod
    def multiband_reference(coeffs, curves, attack, release, x, state=None, want_bands=False):
        return multiband_reference(coeffs, curves, attack, release, x, state, want_bands)

    @staticmethod
    def multiband_design(sample_rate, splits_hz):
        return multiband_design(sample_rate, splits_hz)

    def render_voices(self, frames, sample_rate=SampleRateKhz(48000)):
        """Mix disabled: (shard_voices, frames) float32."""
        out = np.empty((self.shard_voices, frames), dtype=np.float32)
        self._check(self.L.s2r_render_voices(self.h, out.ctypes.data_as(_f32p), frames, int(sample_rate)))
        return out

    def fill_device(self, dev_ptr, frames, sample_rate=SampleRateKhz(48000), stream=None):
        """Partial mix of this shard into device memory at ``dev_ptr`` on ``stream`` (async)."""
        self._check(self.L.s2r_fill_device(self.h, C.c_void_p(dev_ptr), frames, int(sample_rate),
                                           C.c_void_p(stream) if stream else None))

    def fill_device_root(self, dev_ptr, frames, sample_rate=SampleRateKhz(48000), stream=None):
        """Final (root-added) mix of a single-shard synth into device memory (async)."""
        self._check(self.L.s2r_fill_device_root(self.h, C.c_void_p(dev_ptr), frames, int(sample_rate),
                                                C.c_void_p(stream) if stream else None))

    def process_layers(self, layers, frames, sample_rate=SampleRateKhz(48000)):
        """process::process_layer_buf_simd (process.rs:14-49) for layers the caller keeps: `layers` (LAYER_CALL_DTYPE) is
        updated in place (the st::Layer fields); returns (n_layers, frames) float32.  The handle is the workspace."""
        assert layers.dtype == LAYER_CALL_DTYPE and layers.flags["C_CONTIGUOUS"]
        out = np.empty((layers.size, frames), dtype=np.float32)
        self._check(self.L.s2r_process_layers(self.h, layers.ctypes.data, layers.size, out.ctypes.data_as(_f32p), frames, int(sample_rate)))
        return out

    def set_voice_log(self, fn):
        """synth.rs:118's log::debug! as a callback fn(voice_index, note) per note_on; None switches it off"""
        self._voice_log = VOICE_LOG_FN((lambda user, i, note: fn(int(i), int(note)))) if fn else VOICE_LOG_FN()
        self._check(self.L.s2r_set_voice_log(self.h, self._voice_log, None))

    # --- state ---
    def export_state(self):
        arr = np.zeros(self.shard_voices, dtype=VOICE_STATE_DTYPE)
        self._check(self.L.s2r_export_state(self.h, arr.ctypes.data))
        return arr

    def import_state(self, arr):
        arr = np.ascontiguousarray(arr, dtype=VOICE_STATE_DTYPE)
        assert arr.size == self.shard_voices
        self._check(self.L.s2r_import_state(self.h, arr.ctypes.data))

    def set_noise_seed(self, voice_index, seed):
        self._check(self.L.s2r_set_noise_seed(self.h, voice_index, seed))

    def set_flat_shortcut(self, enabled=True):
        self._check(self.L.s2r_set_flat_shortcut(self.h, 1 if enabled else 0))

    def set_coeff_stream(self, enabled=True):
        """False/0: filter coefficients computed in-lane; True/1: read from the patch's coefficient tables, few untimed
        events ride in the render kernel's arguments; 2: tables, events always through their own launch; 3 / 4: synonyms
        of 1 / 2"""
        self._check(self.L.s2r_set_coeff_stream(self.h, int(enabled)))

    def set_uniform_window(self, enabled=True):
        """measurement aid (default on): cohort waves read their chunks' uniform inputs from an LDS window; same bits"""
        self._check(self.L.s2r_set_uniform_window(self.h, 1 if enabled else 0))

    def uniform_window_chunks(self):
        """16-frame chunks rendered through the uniform window since the handle was created"""
        n = C.c_uint64(0)
        self._check(self.L.s2r_uniform_window_chunks(self.h, C.byref(n)))
        return int(n.value)

    def set_low_latency(self, enabled=True):
        """a resident render kernel between sample() calls (small pools, s2r.h: s2r_set_low_latency): the reference's own
        16-frames-per-call pattern without a launch per call"""
        self._check(self.L.s2r_set_low_latency(self.h, 1 if enabled else 0))

    @property
    def low_latency_active(self):
        return bool(self.L.s2r_low_latency_active(self.h))

    def set_resident(self, enabled=True):
        """keep the shard's whole render grid on the device between fills (s2r.h: s2r_set_resident): a fill is a posted
        command, not a launch; with two fills in flight the workgroups run ahead of each other"""
        self._check(self.L.s2r_set_resident(self.h, 1 if enabled else 0))

    @property
    def resident_active(self):
        return bool(self.L.s2r_resident_active(self.h))

    def quiesce(self):
        """stop any resident kernel of the handle and wait for it (before a device-wide synchronize)"""
        self._check(self.L.s2r_quiesce(self.h))

    def exchange_create(self, n_ranks):
        """rank 0 of a group of processes (one per GPU): the rows' block; returns the 64 handle bytes for the other ranks"""
        buf = C.create_string_buffer(64)
        self._check(self.L.s2r_exchange_create(self.h, n_ranks, buf, 64))
        return buf.raw

    def exchange_attach(self, rank, n_ranks, handle):
        buf = C.create_string_buffer(bytes(handle), 64)
        self._check(self.L.s2r_exchange_attach(self.h, rank, n_ranks, buf, 64))

    def set_timing(self, enabled=True):
        self._check(self.L.s2r_set_timing(self.h, 1 if enabled else 0))

    def last_render_ms(self):
        return float(self.L.s2r_last_render_ms(self.h))


def sum_partials_device(rows_ptr, n_rows, frames, out_ptr, stream=None):
    """out = (+0.0 + row0) + row1 + ... on device, rank order (multi-GPU root combine)."""
    rc = load_library().s2r_sum_partials_device(C.c_void_p(rows_ptr), n_rows, frames, C.c_void_p(out_ptr),
                                                C.c_void_p(stream) if stream else None)
    if rc != S2R_OK:
        raise S2rError(rc, "s2r_sum_partials_device")
