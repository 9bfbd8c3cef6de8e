"""synth2_amd — MI355X-native voice-render path behind s2_lib's buffer-fill API.

csrc/ holds the HIP kernels and the C ABI (libs2r.so, declared in include/s2r.h);
synth.py is the ctypes mirror of the reference's ``Synth`` used by tests and bench.py.
"""
from .synth import (Adsr, Note, Patch, S2rError, SampleRateKhz, Synth, Velocity, VoicePool,  # noqa: F401
                    default_patch, load_library, parse_patch, shard_pool_indices, stream_frame_json, sum_partials_device,
                    voice_pan, pan_gains, voice_gain, fader_gains, send_gain, reverb_reference, delay_reference, chorus_reference, chorus_history_frames, chorus_rate, eq_reference, eq_design, dynamics_reference, dynamics_curve, dynamics_coef, room_reference, room_design, room_state_floats, drive_reference, drive_curve, drive_taps, flanger_reference, flanger_history_frames, master_reference, limiter_reference, loudness_reference, loudness_readings, loudness_design, spectrum_reference, spectrum_readings, spectrum_band_readings, spectrum_window, spectrum_twiddles, pcm_reference, pcm_dither, pcm_pack, pcm_shaper, resampler_reference, resampler_count, resampler_design, resampler_state_floats, resampler_max_out, multiband_reference, multiband_design, multiband_sections, multiband_state_floats, MULTIBAND_MAX_BANDS, MAX_BUSES, MAX_IR_TAPS, MAX_DELAY_FRAMES, CHORUS_MAX_VOICES, CHORUS_MAX_DELAY, EQ_MAX_BANDS, DYN_CURVE_POINTS, ROOM_COMBS, ROOM_ALLPASSES, ROOM_MIN_DELAY, ROOM_MAX_DELAY, DRIVE_OVERSAMPLE, DRIVE_TAPS, DRIVE_LATENCY, DRIVE_HISTORY, DRIVE_CURVE_POINTS, DRIVE_MAX_PRE, DRIVE_LINEAR, DRIVE_TANH, DRIVE_HARD, DRIVE_CUBIC, DRIVE_FOLD, FLANGER_MIN_DELAY, FLANGER_MAX_DELAY, EQ_PEAK, EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_LOWPASS, EQ_HIGHPASS, IR_SEGMENT, METER_BLOCK,
                    LIMITER_MAX_LOOKAHEAD, LIMITER_MAX_HOLD, LIMITER_CEILING_LOG2,
                    limiter_tp_reference, LIMITER_SAMPLE_PEAK, LIMITER_TRUE_PEAK, LIMITER_TP_LATENCY, LIMITER_TP_HISTORY,
                    LOUDNESS_PROGRAMMES, LOUDNESS_CHANNELS, LOUDNESS_STATE, LOUDNESS_MIN_HOP, LOUDNESS_MAX_HOP, LOUDNESS_MIN_HOPS, LOUDNESS_MAX_HOPS,
                    SPECTRUM_PROGRAMMES, SPECTRUM_MIN_FFT, SPECTRUM_MAX_FFT, SPECTRUM_MIN_HOP, SPECTRUM_MAX_HOP, SPECTRUM_MAX_ROWS, WINDOW_RECT, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN_HARRIS,
                    PCM_PROGRAMMES, PCM_CHANNELS, PCM_MAX_TAPS, PCM_STATE, PCM_MIN_BITS, PCM_MAX_BITS, PCM_MAX_TAP, DITHER_NONE, DITHER_RECT, DITHER_TRI,
                    RESAMPLER_PROGRAMMES, RESAMPLER_CHANNELS, RESAMPLER_MAX_FACTOR, RESAMPLER_MIN_TAPS, RESAMPLER_MAX_TAPS, RESAMPLER_MAX_TABLE, RESAMPLER_MAX_TAP,
                    SHAPER_FLAT, SHAPER_FIRST, SHAPER_SECOND, SHAPER_3TAP, SHAPER_5TAP, SHAPER_9TAP,
                    OSC_SAW, OSC_SINE, OSC_SQUARE, OSC_TRIANGLE, OSC_DPW_SAW, OSC_DPW_SQUARE, OSC_DPW_TRIANGLE, VOICE_STATE_DTYPE, NOTE_EVENT_DTYPE, LAYER_CALL_DTYPE,
                    FILT_ONEPOLE, FILT_LP1, FILT_HP1, FILT_LP2, FILT_HP2, FILT_BP2,
                    FILT_SVF_LP, FILT_SVF_BP, FILT_SVF_HP)
