"""Builds libs2r.so (the gfx950 voice-render library) in-tree with hipcc.

hipcc cross-compiles gfx950 without a GPU, so this runs in the build container as well as on
the GPU box.  -ffp-contract=off is mandatory (bit-exact arithmetic, see csrc/s2r_math.h).
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libs2r.so")
# One translation unit per oscillator kind for each of the two render kernels: they compile in parallel (the whole
# library in ~40 s on 8 cores instead of ~110 s as one file) and share everything through s2r_kern_common.h.
SOURCES = ["s2r_render_onepole_square.hip", "s2r_render_onepole_saw.hip", "s2r_render_onepole_triangle.hip",
           "s2r_render_onepole_sine.hip", "s2r_render_general_square.hip", "s2r_render_general_saw.hip",
           "s2r_render_general_triangle.hip", "s2r_render_general_sine.hip", "s2r_render_general_bank.hip",
           "s2r_aux.hip", "s2r_eq.hip", "s2r_chorus.hip", "s2r_delay.hip", "s2r_fx.hip", "s2r_master.hip", "s2r_limiter.hip", "s2r_host.cpp", "s2r_post.cpp", "s2r_rules.cpp", "s2r_patch.cpp",
           "s2r_stream.cpp",
           "s2r_dyn.hip",       # (behind the rest: every object in front of it keeps the place in the library it had before the dynamics came)
           "s2r_room.hip",      # (likewise, since the room came)
           "s2r_drive.hip",     # (likewise, since the drive came)
           "s2r_flanger.hip",   # (likewise, since the flanger came)
           "s2r_loudness.hip",  # (likewise, since the loudness meters came)
           "s2r_spectrum.hip",  # (likewise, since the spectrum meters came)
           "s2r_mixer.cpp",     # (likewise, since the voice mixer got a type of its own: host code only, no kernel)
           "s2r_host_mix.cpp",  # (likewise, since the host file was split: host code only, no kernel)
           "s2r_host_post.cpp", # (likewise)
           "s2r_pcm.hip",       # (likewise, since the PCM stage came)
           "s2r_resampler.hip", # (likewise, since the sample-rate converter came)
           "s2r_limiter_tp.hip",    # (likewise, since the limiter's true-peak detector came)
           "s2r_multiband.hip"]     # (last, likewise, since the master's multiband compressor came)
HEADERS = ["s2r_device.h", "s2r_math.h", "s2r_patch.h", "s2r_voices.h", "s2r_kern_common.h", "s2r_render_onepole.inc",
           "s2r_render_general.inc", "s2r_post.h", "s2r_post_route.h", "s2r_post_keep.h", "s2r_rules.h", "s2r_handle.h", "s2r_mixer.h",
           "s2r_mixer_keep.h"]

# -amdgpu-sched-strategy=max-ilp: the render kernels run one wavefront per SIMD (64 k voices =
# 1024 waves), so nothing hides a dependent instruction's latency except independent work of the
# same wave; the default (occupancy-driven) scheduler lines the recurrences up back to back
# (0.086 -> measured below).  Scheduling only: the arithmetic is untouched.
# -O2, not -O3: the same speed (measured on every kernel; the patch-bank kernel is 13 % faster at -O2).  Round 1 recorded
# a wrong result of one variant of the general render kernel at -O3; it belonged to an uncommitted intermediate and has
# not been reproduced since — the committed sources of every round pass the whole GPU suite and the fuzzer at -O3 too
# (S2R_OPT=O3 below builds them that way), so nothing here claims a compiler fault.
FLAGS = ["--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-mllvm", "-amdgpu-sched-strategy=max-ilp",
         "-fPIC", "-Wall", "-Wno-unused-function"]


PER_FILE_FLAGS = {}
# -ftrivial-auto-var-init=zero for the translation units of s2r_render_general.inc: every local that source leaves without a value
# starts as zero bits.  Round 4 met a result that depended on code nowhere near it: the patch bank's pool-resident kernel
# rendered one restarted LP2 voice 7e-4 off after an unrelated block was added to fused_tail — identically at -O0, -O1 and -O2,
# right again after any edit to general_fill (a counter, a printf) and under this flag with either fill pattern; the
# launch-per-fill kernel of the same source was right throughout.  It looks like the read of an indeterminate local, but the
# optimised IR of the =zero and =pattern builds differs in the padding bytes of two structs only: no such read survives to the
# back end, and the cause has NOT been found (CHANGELOG, round 4).  Until it is, these kernels are built with every local
# defined, on which 387 GPU tests and 2 000 fuzz cases are green.  Not for the one-pole kernels (their own source, never seen
# to move): the flag costs the timed kernel 3 % (A/B on one box: 0.0430 -> 0.0446 ms).
for _f in ("s2r_render_general_square.hip", "s2r_render_general_saw.hip", "s2r_render_general_triangle.hip", "s2r_render_general_sine.hip",
           "s2r_render_general_bank.hip"):
    PER_FILE_FLAGS[_f] = ["-ftrivial-auto-var-init=zero"]
# Fifteen translation units are compiled with the back end's resource-usage remarks, and _check_resources() fails the build when a
# kernel named here went to scratch or spilled, or when fewer kernels report than the file instantiates.  Per source file: the
# substrings that name its checked kernels; how many reports are expected — ("at least", n), ("exactly", n), or ("each", None):
# one or more of every name — and why so many; the figures that must be "0"; and what the kernels keep where it belongs.  (The
# bus mixdown's widest forms spill a few SGPRs, which costs nothing that was measured: s2r_aux.hip has no SGPR condition.)
_SCRATCH, _VSPILL, _SSPILL = "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"
RESOURCE_CHECKS = {
    # up to sixteen sums per frame in registers, the bus count compiled in
    "s2r_aux.hip": (("s2r_bus_mix_kernel", "s2r_bus_combine_kernel"),
                    ("at least", 33), "2 load widths x 4 bus counts, static and ramped, without and with aux sends, and the combine",
                    (_SCRATCH, _VSPILL), "its sums must stay in registers"),
    # the convolve kernel slides two windows of samples through registers, fully unrolled
    "s2r_fx.hip": (("s2r_fx_stage_kernel", "s2r_fx_convolve_kernel", "s2r_fx_finish_kernel"), ("each", None), "the reverb's three kernels",
                   (_SCRATCH, _VSPILL, _SSPILL), "its windows and sums must stay in registers"),
    # up to sixteen stem samples and eighteen meter values per thread
    # one band of one channel of one bus per lane: five coefficients, two states, a tile of input loaded ahead
    "s2r_eq.hip": (("s2r_eq_kernel",), ("exactly", 1), "one kernel",
                   (_SCRATCH, _VSPILL, _SSPILL), "its coefficients, states and the tile loaded ahead must stay in registers"),
    # one walker lane with its gain, minimum and sixteen targets; a frame of the key and a frame of the bus per producer / consumer lane
    "s2r_dyn.hip": (("s2r_dyn_kernel",), ("exactly", 1), "one kernel",
                    (_SCRATCH, _VSPILL, _SSPILL), "its gain and the targets read ahead must stay in registers, curve and tiles in LDS"),
    # a frame of one line per lane: the line's frame loaded a tile ahead, a walker's f; a consumer lane's four allpass frames loaded ahead
    "s2r_room.hip": (("s2r_room_kernel",), ("exactly", 1), "one kernel",
                     (_SCRATCH, _VSPILL, _SSPILL), "its frames loaded ahead and the combs' filter values must stay in registers, tiles in LDS"),
    # a frame per lane: both channels' seventeen inputs and four sums in phase 1, two sums in phase 2, half of each filter's taps in
    # SGPRs (156 VGPRs, 102 SGPRs, 14 480 bytes of LDS)
    "s2r_drive.hip": (("s2r_drive_kernel",), ("exactly", 1), "one kernel",
                      (_SCRATCH, _VSPILL, _SSPILL), "its inputs and sums must stay in registers, tiles, table and phase planes in LDS"),
    # a frame of one channel per lane: its two tap addresses, fraction and write address computed a tile ahead, its input loaded
    # four tiles ahead; the line's window of 4096 frames in LDS
    "s2r_flanger.hip": (("s2r_flanger_kernel",), ("exactly", 1), "one kernel",
                        (_SCRATCH, _VSPILL, _SSPILL), "its addresses, fractions and the inputs loaded ahead must stay in registers, the line's window in LDS"),
    # one frame of the chorus per thread: both channels, up to eight voices, two taps each
    "s2r_chorus.hip": (("s2r_chorus_kernel",), ("exactly", 1), "one kernel",
                       (_SCRATCH, _VSPILL, _SSPILL), "its phases, taps and sums must stay in registers"),
    # one residue of the delay per thread: both channels of the line and the loads issued ahead
    "s2r_delay.hip": (("s2r_delay_kernel",), ("exactly", 1), "one kernel",
                      (_SCRATCH, _VSPILL, _SSPILL), "its line pair and the pairs loaded ahead must stay in registers"),
    "s2r_master.hip": (("s2r_master_kernel",), ("exactly", 4), "the bus counts 1, 2, 4 and 8",
                       (_SCRATCH, _VSPILL, _SSPILL), "its stems and meter values must stay in registers"),
    "s2r_limiter.hip": (("s2r_limiter_kernel",), ("exactly", 1), "one kernel",
                        (_SCRATCH, _VSPILL, _SSPILL), "its windows live in LDS, the rest in registers"),
    # a frame per lane: seventeen input frames and two sums per gain, the taps in SGPRs; the gain windows and the input window in LDS
    "s2r_limiter_tp.hip": (("s2r_limiter_tp_kernel",), ("exactly", 1), "one kernel",
                           (_SCRATCH, _VSPILL, _SSPILL), "its frames and sums must stay in registers, its windows in LDS"),
    # a channel per walker lane: ten coefficients, four filter values, the hop sum and sixteen samples read ahead; nine frames of a tile
    # per stager lane; seventeen master frames and two sums per true-peak lane, the taps in SGPRs
    "s2r_loudness.hip": (("s2r_loudness_kernel",), ("exactly", 1), "one kernel",
                         (_SCRATCH, _VSPILL, _SSPILL), "its filter values, sums and the samples read ahead must stay in registers, the tiles in LDS"),
    # eight or sixteen points of one pass per lane and the twiddles of its layers; the transform and the twiddle table in LDS
    "s2r_spectrum.hip": (("s2r_spectrum_kernel",), ("exactly", 1), "one kernel",
                         (_SCRATCH, _VSPILL, _SSPILL), "the points of a pass must stay in registers, the transform and its twiddles in LDS"),
    # a channel per walker lane: nine taps, nine sums and nine errors, sixteen values read ahead; a frame per stager lane: nine frames of
    # a tile, their eighteen dither values
    "s2r_pcm.hip": (("s2r_pcm_kernel",), ("exactly", 1), "one kernel",
                    (_SCRATCH, _VSPILL, _SSPILL), "its sums, errors and the values read ahead must stay in registers, the tiles in LDS"),
    # an output frame per lane: eight accumulators, four taps and four frames of a step
    "s2r_resampler.hip": (("s2r_resampler_kernel",), ("exactly", 1), "one kernel",
                          (_SCRATCH, _VSPILL, _SSPILL), "the four chains of both channels must stay in registers, the rows and the span in LDS"),
    # a section of one channel per crossover lane: five coefficients, two states, eight inputs read ahead, two values on their way; a
    # band per walker lane: its gain, minimum and sixteen targets; a frame per worker lane
    "s2r_multiband.hip": (("s2r_multiband_kernel",), ("exactly", 1), "one kernel",
                          (_SCRATCH, _VSPILL, _SSPILL), "its coefficients, states, gains and the values read ahead must stay in registers, curves, tiles and the bands' ring in LDS"),
}
for _f in RESOURCE_CHECKS:
    PER_FILE_FLAGS[_f] = ["-Rpass-analysis=kernel-resource-usage"]
# s2r_loudness.hip is compiled at -O1.  At -O2 this compiler's code for the kernel's tiled walk computes wrong hop sums and filter values on
# an MI355X — the first frame of a block of eight takes b2 * x where the rule has s1, as far as the assembly was read — with and without
# SLP vectorisation, -fno-strict-aliasing or the max-ilp scheduler, while the optimised IR is the rule's, and the -O1 object and the
# serial form at -O2 are right in every bit (tests/test_gpu_loudness.py).  The cause has NOT been found (CHANGELOG); until it is, -O1.
PER_FILE_FLAGS["s2r_loudness.hip"] = ["drop:-O2", "-O1"] + PER_FILE_FLAGS["s2r_loudness.hip"]
if os.environ.get("S2R_EXPERIMENT_BANK_FLAGS"):                 # (development: extra flags for the patch-bank translation unit)
    PER_FILE_FLAGS["s2r_render_general_bank.hip"] = PER_FILE_FLAGS["s2r_render_general_bank.hip"] + os.environ["S2R_EXPERIMENT_BANK_FLAGS"].split()

# S2R_EQ_SERIAL=1 in the environment builds the EQ kernel's dropped form (one thread runs a channel's whole cascade; csrc/s2r_eq.hip,
# CHANGELOG) into libs2r_eqserial.so, for tools/eq_time.py to time beside the product through S2R_AB_LIB.  Never the product build.
_EQ_SERIAL = os.environ.get("S2R_EQ_SERIAL") == "1"
if _EQ_SERIAL:
    PER_FILE_FLAGS["s2r_eq.hip"] = PER_FILE_FLAGS["s2r_eq.hip"] + ["-DS2R_EQ_SERIAL"]
# S2R_DYN_SERIAL=1 likewise builds the dynamics kernel's dropped form (one thread per bus does all four steps; csrc/s2r_dyn.hip,
# CHANGELOG) into libs2r_dynserial.so, for tools/dyn_time.py.  Never the product build.
_DYN_SERIAL = os.environ.get("S2R_DYN_SERIAL") == "1"
if _DYN_SERIAL:
    PER_FILE_FLAGS["s2r_dyn.hip"] = PER_FILE_FLAGS["s2r_dyn.hip"] + ["-DS2R_DYN_SERIAL"]
# S2R_ROOM_SERIAL=1 likewise builds the room kernel's obvious form (one thread per comb does its own loads, recursion and stores;
# csrc/s2r_room.hip, CHANGELOG) into libs2r_roomserial.so, for tools/room_time.py.  Never the product build.
_ROOM_SERIAL = os.environ.get("S2R_ROOM_SERIAL") == "1"
if _ROOM_SERIAL:
    PER_FILE_FLAGS["s2r_room.hip"] = PER_FILE_FLAGS["s2r_room.hip"] + ["-DS2R_ROOM_SERIAL"]
# S2R_DRIVE_SERIAL=1 likewise builds the drive kernel's obvious form (one lane per output frame recomputes its own 65 oversampled
# samples from global memory, no LDS; csrc/s2r_drive.hip, CHANGELOG) into libs2r_driveserial.so, for tools/drive_time.py; and
# S2R_DRIVE_INTERLEAVED=1 the tiled form with w[] interleaved in LDS instead of in four phase planes, into libs2r_driveinterleaved.so,
# timed once to show what the planes buy.  Never the product build.
_DRIVE_SERIAL = os.environ.get("S2R_DRIVE_SERIAL") == "1"
_DRIVE_INTERLEAVED = not _DRIVE_SERIAL and os.environ.get("S2R_DRIVE_INTERLEAVED") == "1"
if _DRIVE_SERIAL:
    PER_FILE_FLAGS["s2r_drive.hip"] = PER_FILE_FLAGS["s2r_drive.hip"] + ["-DS2R_DRIVE_SERIAL"]
if _DRIVE_INTERLEAVED:
    PER_FILE_FLAGS["s2r_drive.hip"] = PER_FILE_FLAGS["s2r_drive.hip"] + ["-DS2R_DRIVE_INTERLEAVED"]
# S2R_FLANGER_SERIAL=1 likewise builds the flanger kernel's obvious form (one lane per bus and channel steps frame by frame, the line in
# global memory; csrc/s2r_flanger.hip, CHANGELOG) into libs2r_flangerserial.so, for tools/flanger_time.py.  Never the product build.
_FLANGER_SERIAL = os.environ.get("S2R_FLANGER_SERIAL") == "1"
if _FLANGER_SERIAL:
    PER_FILE_FLAGS["s2r_flanger.hip"] = PER_FILE_FLAGS["s2r_flanger.hip"] + ["-DS2R_FLANGER_SERIAL"]
# S2R_LOUDNESS_SERIAL=1 likewise builds the loudness kernel's obvious form (a lane per channel steps through global memory frame by
# frame; csrc/s2r_loudness.hip, CHANGELOG) into libs2r_loudnessserial.so, for tools/loudness_time.py.  Never the product build.
_LOUDNESS_SERIAL = os.environ.get("S2R_LOUDNESS_SERIAL") == "1"
if _LOUDNESS_SERIAL:
    PER_FILE_FLAGS["s2r_loudness.hip"] = PER_FILE_FLAGS["s2r_loudness.hip"] + ["-DS2R_LOUDNESS_SERIAL"]
# S2R_SPECTRUM_SERIAL=1 likewise builds the spectrum kernel's obvious form (a barrier per radix-2 layer, no padding, one point pair per
# thread and layer; csrc/s2r_spectrum.hip, CHANGELOG) into libs2r_spectrumserial.so, for tools/spectrum_time.py.  Never the product build.
_SPECTRUM_SERIAL = os.environ.get("S2R_SPECTRUM_SERIAL") == "1"
if _SPECTRUM_SERIAL:
    PER_FILE_FLAGS["s2r_spectrum.hip"] = PER_FILE_FLAGS["s2r_spectrum.hip"] + ["-DS2R_SPECTRUM_SERIAL"]
# S2R_PCM_SERIAL=1 likewise builds the PCM kernel's obvious form (a lane per channel steps through global memory frame by frame, step 2
# as the rule's loop; csrc/s2r_pcm.hip, CHANGELOG) into libs2r_pcmserial.so, for tools/pcm_time.py.  Never the product build.
_PCM_SERIAL = os.environ.get("S2R_PCM_SERIAL") == "1"
if _PCM_SERIAL:
    PER_FILE_FLAGS["s2r_pcm.hip"] = PER_FILE_FLAGS["s2r_pcm.hip"] + ["-DS2R_PCM_SERIAL"]
# S2R_RESAMPLER_SERIAL=1 likewise builds the resampler kernel's obvious form (every lane reads its table row and its input frames from
# global memory; csrc/s2r_resampler.hip, CHANGELOG) into libs2r_resamplerserial.so, for tools/resampler_time.py.  Never the product build.
_RESAMPLER_SERIAL = os.environ.get("S2R_RESAMPLER_SERIAL") == "1"
if _RESAMPLER_SERIAL:
    PER_FILE_FLAGS["s2r_resampler.hip"] = PER_FILE_FLAGS["s2r_resampler.hip"] + ["-DS2R_RESAMPLER_SERIAL"]
# S2R_LIMITER_TP_NAIVE=1 likewise builds the true-peak limiter's obvious form (each thread sums its gains straight from global memory, no
# input window in LDS; csrc/s2r_limiter_tp.hip, CHANGELOG) into libs2r_limitertpnaive.so, for tools/limiter_time.py --true-peak.  Never
# the product build.
_LIMITER_TP_NAIVE = os.environ.get("S2R_LIMITER_TP_NAIVE") == "1"
if _LIMITER_TP_NAIVE:
    PER_FILE_FLAGS["s2r_limiter_tp.hip"] = PER_FILE_FLAGS["s2r_limiter_tp.hip"] + ["-DS2R_LIMITER_TP_NAIVE"]
# S2R_MULTIBAND_SERIAL=1 likewise builds the multiband kernel's obvious form (a lane per channel runs every section of a frame and then
# the four gains, from global memory; csrc/s2r_multiband.hip, CHANGELOG) into libs2r_multibandserial.so, for tools/multiband_time.py.
# Never the product build.
_MULTIBAND_SERIAL = os.environ.get("S2R_MULTIBAND_SERIAL") == "1"
if _MULTIBAND_SERIAL:
    PER_FILE_FLAGS["s2r_multiband.hip"] = PER_FILE_FLAGS["s2r_multiband.hip"] + ["-DS2R_MULTIBAND_SERIAL"]
    # (the comparison form reads 75 uniform coefficients at its head and spills 8 SGPRs there, outside its frame loop: no SGPR condition)
    RESOURCE_CHECKS["s2r_multiband.hip"] = RESOURCE_CHECKS["s2r_multiband.hip"][:3] + ((_SCRATCH, _VSPILL),) + RESOURCE_CHECKS["s2r_multiband.hip"][4:]
# S2R_OPT=O3 in the environment builds the same sources at -O3 into libs2r_o3.so (tools and tests that compare the two
# optimisation levels; the product is -O2).
if os.environ.get("S2R_OPT") == "O3":
    FLAGS = [("-O3" if f == "-O2" else f) for f in FLAGS]
    LIB = os.path.join(HERE, "libs2r_o3.so")
# S2R_STAMPS=1 in the environment builds the DIAGNOSTIC library (its own file, libs2r_stamps.so): the one-pole render
# kernel writes s_memtime stamps at its phase boundaries (tools/stamps.py).  Never the product build.
if os.environ.get("S2R_STAMPS") == "1":
    FLAGS = FLAGS + ["-DS2R_STAMPS"]
    LIB = os.path.join(HERE, "libs2r_stamps.so")
    OBJ_DIR_NAME = "_build_stamps"
elif os.environ.get("S2R_OPT") == "O3":
    OBJ_DIR_NAME = "_build_o3"
elif _EQ_SERIAL:
    LIB = os.path.join(HERE, "libs2r_eqserial.so")
    OBJ_DIR_NAME = "_build_eqserial"
elif _DYN_SERIAL:
    LIB = os.path.join(HERE, "libs2r_dynserial.so")
    OBJ_DIR_NAME = "_build_dynserial"
elif _ROOM_SERIAL:
    LIB = os.path.join(HERE, "libs2r_roomserial.so")
    OBJ_DIR_NAME = "_build_roomserial"
elif _DRIVE_SERIAL:
    LIB = os.path.join(HERE, "libs2r_driveserial.so")
    OBJ_DIR_NAME = "_build_driveserial"
elif _DRIVE_INTERLEAVED:
    LIB = os.path.join(HERE, "libs2r_driveinterleaved.so")
    OBJ_DIR_NAME = "_build_driveinterleaved"
elif _FLANGER_SERIAL:
    LIB = os.path.join(HERE, "libs2r_flangerserial.so")
    OBJ_DIR_NAME = "_build_flangerserial"
elif _LOUDNESS_SERIAL:
    LIB = os.path.join(HERE, "libs2r_loudnessserial.so")
    OBJ_DIR_NAME = "_build_loudnessserial"
elif _SPECTRUM_SERIAL:
    LIB = os.path.join(HERE, "libs2r_spectrumserial.so")
    OBJ_DIR_NAME = "_build_spectrumserial"
elif _PCM_SERIAL:
    LIB = os.path.join(HERE, "libs2r_pcmserial.so")
    OBJ_DIR_NAME = "_build_pcmserial"
elif _RESAMPLER_SERIAL:
    LIB = os.path.join(HERE, "libs2r_resamplerserial.so")
    OBJ_DIR_NAME = "_build_resamplerserial"
elif _LIMITER_TP_NAIVE:
    LIB = os.path.join(HERE, "libs2r_limitertpnaive.so")
    OBJ_DIR_NAME = "_build_limitertpnaive"
elif _MULTIBAND_SERIAL:
    LIB = os.path.join(HERE, "libs2r_multibandserial.so")
    OBJ_DIR_NAME = "_build_multibandserial"
else:
    OBJ_DIR_NAME = "_build"


OBJ_DIR = os.path.join(HERE, OBJ_DIR_NAME)
# S2R_AB_LIB=<path>: development aid for A/B timing on one GPU box — loads a library kept from another build of these
# sources (same ABI) instead of libs2r.so; never rebuilt, never the product.
AB_LIB = os.environ.get("S2R_AB_LIB")
if AB_LIB:
    LIB = os.path.abspath(AB_LIB)


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libs2r cannot be built (there is no CPU fallback)")


def source_hash(csrc=None):
    """identifies the sources a library was built from: sha256 over the names and bytes of csrc/'s sources (bench.py's
    kernel_source_hash is this function; the committed rocprofv3 summaries under profiles/ carry it)"""
    csrc = csrc or CSRC
    h = hashlib.sha256()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".inc", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


def build_id(csrc=None):
    """what s2r_build_id() of a library built NOW would return: <source hash>-<hash of include/s2r.h and the flags>"""
    h = hashlib.sha256()
    h.update(open(os.path.join(ROOT, "include", "s2r.h"), "rb").read())
    h.update(repr(FLAGS).encode())
    h.update(repr(sorted(PER_FILE_FLAGS.items())).encode())
    return source_hash(csrc) + "-" + h.hexdigest()[:8]


_ID_MARK = b"S2R_BUILD_ID="


def embedded_build_id(lib=None):
    """the build id compiled into a libs2r.so (s2r_build_id(), read from the file without loading it), or None"""
    try:
        data = open(lib or LIB, "rb").read()
    except OSError:
        return None
    m = re.search(re.escape(_ID_MARK) + rb"([0-9a-f]{16}-[0-9a-f]{8})", data)
    return m.group(1).decode() if m else None


def needs_build(csrc=None):
    """The library is bound to its sources by CONTENT: it carries the hash of the sources it was built from
    (s2r_build_id), and anything else on disk — whatever the files' times say — is a stale binary."""
    if AB_LIB:
        if not os.path.exists(LIB):
            raise RuntimeError("S2R_AB_LIB=%s does not exist" % LIB)
        return False
    if not os.path.exists(LIB):
        return True
    return embedded_build_id() != build_id(csrc)


def _compile_one(args):
    cc, src, obj, verbose, extra, stamp = args
    flags = list(FLAGS)
    for drop in [x[len("drop:"):] for x in extra if x.startswith("drop:")]:     # (development: "drop:<flag>" among a file's extra flags removes it)
        flags = [f for f in flags if f != drop]
    drops = [x[len("drop:"):] for x in extra if x.startswith("drop:")]
    extra = [x for x in extra if not x.startswith("drop:") and x not in drops]
    cmd = [cc] + flags + extra + ["-x", "hip", "-c", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", obj, src]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    if "-Rpass-analysis=kernel-resource-usage" in extra:
        r = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            raise subprocess.CalledProcessError(r.returncode, cmd)
        usage = kernel_resources(r.stderr)
        with open(os.path.splitext(obj)[0] + ".resources.txt", "w") as f:
            for name, u in usage:
                f.write("%s: %s\n" % (name, ", ".join("%s %s" % kv for kv in u.items())))
        _check_resources(os.path.basename(src), usage)
    else:
        subprocess.check_call(cmd)
    with open(obj + ".id", "w") as f:
        f.write(stamp)
    return obj


def kernel_resources(remarks):
    """[(mangled kernel name, {figure: value})] from the text of -Rpass-analysis=kernel-resource-usage"""
    out = []
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            out.append((val, {}))
        elif out:
            out[-1][1][key] = val
    return out


def _check_resources(source, usage):
    if source not in RESOURCE_CHECKS:
        raise RuntimeError("libs2r: %s is compiled with the resource-usage remarks and has no entry in RESOURCE_CHECKS" % source)
    names, (rule, count), why_count, zero, why = RESOURCE_CHECKS[source]
    seen = []
    for name, u in usage:
        for k in names:
            if k in name:
                seen.append(k)
                bad = [figure for figure in zero if u.get(figure) != "0"]
                if bad:
                    raise RuntimeError("libs2r: %s has a non-zero %s (%r): %s" % (name, ", ".join(bad), u, why))
    if rule == "each":
        ok, n = set(seen) == set(names), len(set(seen))
    else:
        ok, n = (len(seen) >= count if rule == "at least" else len(seen) == count), len(seen)
    if not ok:
        raise RuntimeError("libs2r: %s: resource usage of %d kernels (%s) reported, %s expected (%s)"
                           % (source, n, ", ".join(sorted(set(seen))), "every one of %s" % list(names) if rule == "each" else "%s %d" % (rule, count), why_count))


def check_m0_contract(lib=None, texts=None):
    """The kernels' tile stores are inline assembly that writes M0 once per chunk (tile_set_base) and reads it in sixteen
    ds_write_addtid_b32 — with no "m0" in the clobber lists (s2r_kern_common.h says why).  That is only sound while nothing the
    compiler emits touches M0 in those kernels, which is a property of THIS compiler on THIS code: so it is checked on the
    disassembly of every library the build links (a compiler that starts using M0 fails the build, here and on any box that
    builds the library, instead of corrupting the mix where the CPU tests are not run first).  Returns (M0 writes, tile
    stores), or None when there is no llvm-objdump to ask.  `texts`: disassembly to check instead of the library's (the test of the
    check itself)."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("s2r_code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if texts is None:
        if not os.path.exists(co.OBJDUMP):
            return None
        texts = co.disassemble(lib or LIB)
    n_set = n_store = 0
    for text in texts:
        lines = [l.split("//")[0].strip() for l in text.splitlines()]
        for i, l in enumerate(lines):
            if "ds_write_addtid_b32" in l:
                n_store += 1
            elif re.search(r"\bm0\b", l):
                if not re.match(r"s_mov_b32 m0, s\d+$", l):
                    raise RuntimeError("libs2r: the compiler uses M0 (%r): the tile stores' inline assembly is no longer safe" % l)
                if not lines[i + 1].startswith("s_nop"):
                    raise RuntimeError("libs2r: M0 written without the wait state in front of the LDS store (%r)" % lines[i + 1])
                n_set += 1
    if not n_set or n_store != 16 * n_set:
        raise RuntimeError("libs2r: %d M0 writes for %d tile stores (sixteen per write expected)" % (n_set, n_store))
    return n_set, n_store


def build(force=False, verbose=False, jobs=None):
    if not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    cc = _hipcc()
    os.makedirs(OBJ_DIR, exist_ok=True)
    bid = build_id()
    # an object is as good as the bytes it was compiled from: its own source, every header, the flags (content, not times)
    hh = hashlib.sha256()
    for f in HEADERS:
        hh.update(open(os.path.join(CSRC, f), "rb").read())
    hh.update(open(os.path.join(ROOT, "include", "s2r.h"), "rb").read())
    hh.update(repr(FLAGS).encode())
    todo, objs = [], []
    for f in SOURCES:
        src, obj = os.path.join(CSRC, f), os.path.join(OBJ_DIR, os.path.splitext(f)[0] + ".o")
        objs.append(obj)
        # (s2r_host.cpp carries the build id: S2R_BUILD_ID, the marker embedded_build_id() looks for)
        extra = ['-DS2R_BUILD_ID="%s"' % bid] if f == "s2r_host.cpp" else list(PER_FILE_FLAGS.get(f, []))
        h = hh.copy(); h.update(open(src, "rb").read()); h.update(repr(extra).encode())
        stamp = h.hexdigest()
        try:
            have = open(obj + ".id").read()
        except OSError:
            have = None
        if force or not os.path.exists(obj) or have != stamp:
            todo.append((cc, src, obj, verbose, extra, stamp))
    jobs = jobs or max(1, min(len(todo), os.cpu_count() or 1, 8))
    if todo:
        with ThreadPoolExecutor(max_workers=jobs) as ex:
            list(ex.map(_compile_one, todo))
    link = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(link), file=sys.stderr)
    subprocess.check_call(link)
    if embedded_build_id() != bid:
        raise RuntimeError("the linked library does not carry the build id %s" % bid)
    try:
        if os.environ.get("S2R_DEBUG_NO_M0_CHECK") != "1":       # (debugging builds with printf in a kernel: the host call uses M0)
            check_m0_contract()
    except RuntimeError:
        os.replace(LIB, LIB + ".rejected")                      # (never loadable under its own name)
        raise
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
