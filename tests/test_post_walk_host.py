"""What the seeded walks of tests/post_walk.py cover, and that the chain's host model alone is well behaved over them — on the CPU, over
the default seeds of tests/test_gpu_post_fuzz.py.  The coverage conditions are conditions on the inputs: the generator's weights and the
default seed count are chosen so that they hold, and this file asserts them.  Conditions 1 to 7 are the chain's, 8 to 16 the meters'
and 17 to 23 those of the stages of DESIGN.md 4.28 to 4.31 (output_survey: on the books, with ph, t and the capacity of the pinned
samples kept as S2rPostChain keeps them); two digests hold the steps of the first generator, and of the first two, to what they were
before the later ones were spliced in; and the models alone must work: the multiband's bands in both branches, the true-peak
detector interpolating and limiting, the PCM stage clipping on both rails but not everywhere and its shaper showing, the converter
making outputs with a bit set, over the default seeds and over both systematic walks."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import post_walk as pw
from post_walk import FILLS, INSERTS, STAGES, STEMS, TWIN_PEAK, Chain, walk
from test_gpu_loudness import BLOCK, walker_distances

F = np.float32
BASE = int(os.environ.get("S2R_POST_FUZZ_BASE", str(pw.DEFAULT_BASE)))
SEEDS = [BASE + k for k in range(int(os.environ.get("S2R_POST_FUZZ_SEEDS", str(pw.DEFAULT_SEEDS))))]
DEFAULTS = [pw.DEFAULT_BASE + k for k in range(pw.DEFAULT_SEEDS)]     # the coverage is claimed of these, wherever the sweep has been moved


def _subsets(names):
    return [frozenset(c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]


def survey(seeds):
    """the walks on the books alone — which effect is present when, no arithmetic — -> what the conditions below ask about"""
    s = dict(kinds=set(), fills=set(), stage_events={st: set() for st in STAGES}, inserts=set(), stems={"bus": set(), "master": set()}, n_buses=set(),
             frames=set(), max_frames=set(), timing=set(), handovers=0, roundtrips=0, idle_between_runs=False, entries=set(), big_room=False,
             flanger=dict(frames=set(), H=set(), idle_between_runs=False, roundtrips=0, handovers=0))
    for seed in seeds:
        setup, steps = walk(seed)
        chain_steps = [a for a in steps if a["kind"] in pw.CHAIN_KINDS]      # (the counts are of these, as before the meters joined)
        assert 20 <= len(chain_steps) <= 30 and sum(a["kind"] == "fill" for a in chain_steps) >= 12, seed
        assert steps[-1]["kind"] == "fill" and steps[-1]["fill"] in ("master", "master_stems"), seed
        assert sum(a["kind"] == "handover" for a in steps) <= 1, seed
        s["max_frames"].add(setup["max_frames"])
        s["timing"].add(setup["timing"])
        present = {st: {} for st in STAGES}                      # stage -> bus -> the key bus (dynamics) or None
        ran, idled = set(), set()                                # (stage, bus) that some fill ran; that a later fill then left idle
        shapes = {}                                              # bus -> the shape its flanger was set with
        for a in steps:
            kind = a["kind"]
            s["kinds"].add(kind)
            if kind == "set":
                assert a["replaces"] == (a["bus"] in present[a["stage"]]), seed
                s["stage_events"][a["stage"]].add("replace" if a["replaces"] else "set")
                present[a["stage"]][a["bus"]] = a["shape"].get("key")
                if a["stage"] == "flanger":
                    shapes[a["bus"]] = a["shape"]
                ran.discard((a["stage"], a["bus"])); idled.discard((a["stage"], a["bus"]))      # a new effect: nothing carried
            elif kind == "clear":
                s["stage_events"][a["stage"]].add("clear")
                del present[a["stage"]][a["bus"]]
                ran.discard((a["stage"], a["bus"])); idled.discard((a["stage"], a["bus"]))
            elif kind == "params":
                assert a["bus"] in present[a["stage"]], seed
                s["stage_events"][a["stage"]].add("params")
                s["entries"].add(a["entry"])
                if a["stage"] == "dyn":
                    present["dyn"][a["bus"]] = a["shape"]["key"]
            elif kind == "handover":
                s["handovers"] += 1
                s["flanger"]["handovers"] += bool(present["flanger"])
            elif kind == "roundtrip":
                s["roundtrips"] += 1
                s["flanger"]["roundtrips"] += bool(present["flanger"])
            elif kind == "fill":
                s["fills"].add(a["fill"])
                assert 1 <= a["frames"] <= setup["max_frames"], seed
                s["frames"] |= {a["frames"]} | {name for name, d in (("max_frames", 0), ("max_frames - 1", 1)) if a["frames"] == setup["max_frames"] - d}
                if a["fill"] == "panned":
                    assert a["n_buses"] == 0
                    continue
                nb = a["n_buses"]
                s["n_buses"].add(nb)

                def active(st, b):                               # as S2rPostChain::prepare decides it
                    return b < nb and (st != "dyn" or present[st][b] < nb)
                on = {st for st in STAGES if any(active(st, b) for b in present[st])}
                s["inserts"].add(frozenset(on & set(INSERTS)))
                s["stems"]["bus" if a["fill"] == "bus" else "master"].add(frozenset(on & set(STEMS)))
                if "room" in on and a["frames"] > 1024:
                    s["big_room"] = True
                for st in STAGES:
                    for b in present[st]:
                        if active(st, b):
                            if (st, b) in idled:
                                s["idle_between_runs"] = True
                                if st == "flanger":
                                    s["flanger"]["idle_between_runs"] = True
                            if st == "flanger":
                                s["flanger"]["frames"].add(a["frames"])
                                s["flanger"]["H"].add(shapes[b]["H"])
                            ran.add((st, b))
                        elif (st, b) in ran and b >= nb:         # present on a bus past the call's, after a fill that ran it
                            idled.add((st, b))
    return s


def test_a_walk_is_a_pure_function_of_its_seed():
    for seed in SEEDS[:8]:
        assert walk(seed) == walk(seed)
    assert walk(SEEDS[0]) != walk(SEEDS[0] + 1)
    assert pw.subset_walk() == pw.subset_walk() and pw.master_subset_walk() == pw.master_subset_walk()


def test_the_default_walks_cover_what_they_are_for():
    s = survey(DEFAULTS)
    # 1. every kind of action, every kind of fill
    assert s["kinds"] == set(pw.KINDS_OF_ACTION), set(pw.KINDS_OF_ACTION) - s["kinds"]
    assert s["fills"] == set(FILLS)
    # 2. every stage is set, cleared, replaced while present and given kept-state parameters, through every kept-state entry
    for st in STAGES:
        assert s["stage_events"][st] == {"set", "clear", "replace", "params"}, (st, s["stage_events"][st])
    assert s["entries"] == {"set_bus_eq_coeffs", "set_bus_dynamics_params", "set_bus_drive_params", "set_bus_room_params", "set_bus_chorus_rate",
                            "set_bus_chorus_mix", "set_bus_delay_mix", "set_bus_reverb_mix", "set_bus_flanger_params"}
    # 3. all 32 subsets of the five inserts are active in some fill; all 8 of the stem stages in a bus fill and in a master fill
    assert len(_subsets(INSERTS)) == 32
    assert s["inserts"] == set(_subsets(INSERTS)), sorted(map(sorted, set(_subsets(INSERTS)) - s["inserts"]))
    for kind in ("bus", "master"):
        assert s["stems"][kind] == set(_subsets(STEMS)), (kind, sorted(map(sorted, set(_subsets(STEMS)) - s["stems"][kind])))
    # 4. every n_buses; an effect idles past the call's buses between two fills that run it
    assert s["n_buses"] == set(range(1, 9))
    assert s["idle_between_runs"]
    # 5. every frame count, every max_frames, timing on and off
    assert s["frames"] >= set(pw.FRAMES) | {"max_frames - 1", "max_frames"}, (set(pw.FRAMES) | {"max_frames - 1", "max_frames"}) - s["frames"]
    assert s["max_frames"] == set(pw.MAX_FRAMES)
    assert s["timing"] == {False, True}
    # 6. a handover, three state round trips
    assert s["handovers"] >= 1 and s["roundtrips"] >= 3
    # and a room runs in a call of more than 1024 frames: its work area's stride is max_frames, not 1024
    assert s["big_room"]
    # 7. the flanger where its kernel can go wrong by itself (s2r_flanger.hip): past the first copy workgroup's 1024 frames and the
    # staging buffer's first 1024; the whole ring; a group of eight tiles that ends the call, one frame less and one more; and between
    # two fills that run it, a fill whose buses end before its bus: no phase advanced, no line flipped (s2r_post.cpp: commit)
    fl = s["flanger"]
    assert any(n > 1024 for n in fl["frames"]), "no flanger runs in a call of more than 1024 frames"
    assert 4096 in fl["H"], "no flanger of H = 4096 runs"
    assert fl["frames"] >= {255, 256, 257}, "no flanger runs in a call of %s frames" % sorted({255, 256, 257} - fl["frames"])
    assert fl["idle_between_runs"], "no flanger idles past the call's buses between two fills that run it"
    assert fl["roundtrips"] >= 1 and fl["handovers"] >= 1, "a flanger's state goes through %d round trips and %d handovers" % (fl["roundtrips"], fl["handovers"])


# sha256 of json.dumps([setup, steps], sort_keys=True), its first 12 digits, of walk(seed) for the 32 default seeds, computed at commit
# f757cfa — the last one before the meters joined the walks, when every step was of CHAIN_KINDS
CHAIN_STEPS_DIGESTS = (
    "59a64a533536", "4e6d7eeda456", "3cfe4c0845c7", "a9f5c0d130ed", "65a61f0d9ba0", "b774507e0f50", "51ef85b77561", "2fb401e058dc",
    "20f0f8799722", "ec95aa516ca7", "72020063398b", "f3a6b3acb4b0", "482a164a904c", "c626d0658bf6", "3d76e8420cd1", "020a99b66ca9",
    "4c20ec6603af", "3779fed92e31", "a33b17dfab49", "05f509eb309c", "20135c851ec2", "a68f720aa7ce", "eacc442e1e10", "f746b734883b",
    "1e61c9ab1d37", "816e3ba3820b", "4187f5fa702d", "41668bf85699", "a3becf003b90", "e2959b7bc2c1", "867942b89cf3", "fd880923ac8f")


def test_the_chain_steps_of_the_default_seeds_are_what_they_were():
    """the meters' actions are spliced between the steps a seed has always given: with them taken out, walk(seed) is the walk of the
    commit before, step for step — the seeds with a history in tests/test_gpu_post_fuzz.py's docstring, and the 1200 recorded there as
    clean, still name the walks they named"""
    assert len(CHAIN_STEPS_DIGESTS) == len(DEFAULTS) == 32
    for seed, want in zip(DEFAULTS, CHAIN_STEPS_DIGESTS):
        setup, steps = walk(seed)
        assert any(a["kind"] in pw.METER_KINDS for a in steps), seed
        chain_steps = [a for a in steps if a["kind"] in pw.CHAIN_KINDS]
        assert hashlib.sha256(json.dumps([setup, chain_steps], sort_keys=True).encode()).hexdigest()[:12] == want, seed


# the same digest of [setup, the steps of CHAIN_KINDS and METER_KINDS], computed at commit 9ee2a99 — the last one before the stages of
# DESIGN.md 4.28 to 4.31 joined the walks, when every step was of those two
METER_STEPS_DIGESTS = (
    "9d49ef37ba15", "c71a4627f9ce", "0bf3d750bc8b", "712b5394284e", "ef9e4b071aa1", "e1fcf797e049", "4ce7f1d18347", "f75123c9e873",
    "5e2f8921c3c6", "32a83e23d32b", "a81ce66a6427", "258634b8cb53", "bedaa9e07af6", "44a7dae44c8d", "105144605d3a", "06f5d00fef12",
    "c8d1c5766380", "164450ee9800", "f54299186d39", "3b44f9cba793", "136c4638fd8c", "dc3e94b5e80f", "729f1e87ea66", "ed964a05487f",
    "7afd9a9dae06", "ab09d1dd6fd0", "906d287cfda4", "59f37ee18a6c", "0aa2c2a2509c", "6bd4ceccc5ce", "675a5a2096e5", "53d4ad49382e")


def test_the_chain_and_meter_steps_of_the_default_seeds_are_what_they_were():
    """the actions of OUTPUT_KINDS are spliced between the steps of the two generators before them: with them taken out, walk(seed) is
    the walk of the commit before, step for step — the 1600 walks recorded as clean in tests/test_gpu_post_fuzz.py's docstring, and
    the seeds with a history there, still name the walks they named"""
    assert len(METER_STEPS_DIGESTS) == len(DEFAULTS) == 32
    for seed, want in zip(DEFAULTS, METER_STEPS_DIGESTS):
        setup, steps = walk(seed)
        assert any(a["kind"] in pw.OUTPUT_KINDS for a in steps), seed
        assert all(a["kind"] in pw.KINDS_OF_ACTION for a in steps), seed
        before = [a for a in steps if a["kind"] in pw.CHAIN_KINDS + pw.METER_KINDS]
        assert hashlib.sha256(json.dumps([setup, before], sort_keys=True).encode()).hexdigest()[:12] == want, seed


class Book:
    """a meter on the books: what its position, its stored rows and the rows it has made are after calls of given lengths"""

    def __init__(self, name, action, serial):
        self.name, self.hop, self.serial = name, action["hop"], serial
        self.keep = action["max_hops"] if name == "loudness" else action["max_rows"]
        self.n_fft = action.get("n_fft")
        self.replaced_another_size = False
        self.restart()

    def restart(self):
        self.pos = self.stored = self.made = 0
        self.calls = []                                          # the frames of the master fills since it started afresh
        self.sat = set()                                         # the fills it has sat through since the last master fill

    def feed(self, frames):
        k = (self.pos + frames) // self.hop
        self.pos, self.made, self.stored = (self.pos + frames) % self.hop, self.made + k, min(self.keep, self.stored + k)
        self.calls.append(frames)
        return k


def meter_survey(seeds):
    """the meters of the walks on the books alone -> what the conditions of test_the_default_walks_cover_the_meters ask about"""
    both = ("loudness", "spectrum")
    s = dict(sizes_with_a_row=set(), replaced_and_compared=False, limiter_and_both=False, without_stems=set(), roundtrips={m: 0 for m in both},
             handovers={m: 0 for m in both}, big={m: False for m in both}, overflow=False, short=False, sat_through_both=False, blocks_at_17=0,
             met_at_17=set(), fill_behind_fill=False, fill_behind_read=set(), refused_with_a_meter=0, hops=set(), max_hops=set(), spectrum_hops=set(),
             windows=set(), max_rows=set(), replaced={m: 0 for m in both}, reset_with_rows={m: 0 for m in both})
    for seed in seeds:
        setup, steps = walk(seed)
        on, limiter, serial = {}, False, 0                       # name -> Book
        last = None                                              # what the state's copies met last: a master "fill", the kind of step that read them, or None
        for k, a in pw.expanded(steps):                          # (a pause of the meters as the clears and sets it stands for)
            kind = a["kind"]
            now = None
            if kind in ("loudness_set", "spectrum_set"):
                name = kind.split("_")[0]
                assert a["replaces"] == (name in on), seed
                serial += 1
                book = Book(name, a, serial)
                if name in on:
                    s["replaced"][name] += 1
                    book.replaced_another_size = name == "spectrum" and on[name].n_fft != a["n_fft"]
                on[name] = book
                if name == "loudness":
                    s["hops"].add(a["hop"]); s["max_hops"].add(a["max_hops"])
                else:
                    assert a["hop"] in pw._spectrum_hops(a["n_fft"]) and a["hop"] >= max(32, a["n_fft"] // 8), seed
                    s["spectrum_hops"].add(pw._spectrum_hops(a["n_fft"]).index(a["hop"])); s["windows"].add(a["window"]); s["max_rows"].add(a["max_rows"])
            elif kind in ("loudness_reset", "spectrum_reset"):
                name = kind.split("_")[0]
                s["reset_with_rows"][name] += on[name].stored > 0
                on[name].restart()
            elif kind in ("loudness_clear", "spectrum_clear"):
                del on[kind.split("_")[0]]
            elif kind == "refused_fill":
                assert a["frames"] == setup["max_frames"] + 1 and 1 <= a["n_buses"] <= 8, seed
                s["refused_with_a_meter"] += bool(on)
                now = last                                       # (it must move nothing: what the next fill meets is what it would have met)
            elif kind in ("limiter_set", "limiter_clear"):
                limiter = kind == "limiter_set"
            elif kind in ("roundtrip", "handover"):
                for name, book in on.items():
                    if book.pos != 0 and book.stored >= 1:
                        s[kind + "s"][name] += 1
                now = kind if on else None
            elif kind == "fill" and a["fill"] in ("bus", "panned"):
                for book in on.values():
                    if book.calls:
                        book.sat.add(a["fill"])
                now = a["fill"] if on and pw.peeks(k) else last
            elif kind == "fill":
                n = a["frames"]
                if on and last == "fill":
                    s["fill_behind_fill"] = True
                if on and last not in (None, "fill"):
                    s["fill_behind_read"].add(last)
                if limiter and len(on) == 2:
                    s["limiter_and_both"] = True
                for name, book in on.items():
                    if a["fill"] == "master":
                        s["without_stems"].add(name)
                    if book.sat >= {"bus", "panned"}:
                        s["sat_through_both"] = True
                    book.sat = set()
                    made = book.feed(n)
                    s["big"][name] |= n > 1024
                    s["overflow"] |= made > book.keep
                    s["short"] |= n < book.hop and made == 0
                    if name == "spectrum" and made:
                        s["sizes_with_a_row"].add(book.n_fft)
                        s["replaced_and_compared"] |= book.replaced_another_size
                    if name == "loudness" and book.hop == 17:
                        met, blocks, pos = walker_distances(17, book.calls)
                        assert pos == book.pos
                        if blocks > s["blocks_at_17"]:
                            s["blocks_at_17"], s["met_at_17"] = blocks, met
                now = "fill" if on else None
            else:
                now = last                                       # (no entry of the chain in front touches the meters' copies)
            last = now
    return s


def test_the_default_walks_cover_the_meters():
    """the conditions on the second generator (post_walk._splice), asserted the way the chain's are: its weights are chosen so that they
    hold over the default seeds"""
    s = meter_survey(DEFAULTS)
    # 8. every shape the meters are drawn in; each of the six transform sizes is set in some walk and completes a row there
    assert s["hops"] == set(pw.LOUDNESS_HOPS) and s["max_hops"] == set(pw.LOUDNESS_MAX_HOPS)
    assert s["spectrum_hops"] == {0, 1, 2} and s["windows"] == set(pw.SPECTRUM_WINDOWS) and s["max_rows"] == set(pw.SPECTRUM_MAX_ROWS)
    assert s["sizes_with_a_row"] == set(pw.SPECTRUM_N), set(pw.SPECTRUM_N) - s["sizes_with_a_row"]
    # 9. a meter is set while one is present, reset with rows stored, and a spectrum meter is replaced by one of another size, whose rows
    # a master fill then completes: the state's copies are reserved anew (s2r_post_keep.h: S2rMirror)
    assert all(s["replaced"].values()) and all(s["reset_with_rows"].values()), (s["replaced"], s["reset_with_rows"])
    assert s["replaced_and_compared"]
    # 10. the limiter and both meters in one master fill; a meter in a master fill without stems
    assert s["limiter_and_both"] and s["without_stems"] == {"loudness", "spectrum"}
    # 11. each meter goes through a round trip and a handover in the middle of a hop with rows stored
    assert all(s["roundtrips"].values()) and all(s["handovers"].values()), (s["roundtrips"], s["handovers"])
    # 12. each meter in a call of more than 1024 frames; a call that completes more rows than the window keeps; a call shorter than the
    # hop that completes none
    assert all(s["big"].values()), s["big"]
    assert s["overflow"] and s["short"]
    # 13. a meter that has run sits through a bus fill and a panned fill before the next master fill
    assert s["sat_through_both"]
    # 14. one loudness meter at hop 17 runs at least 17 full blocks of eight frames, and starts one eight frames before the hop's end
    assert s["blocks_at_17"] >= 17 and BLOCK in s["met_at_17"], (s["blocks_at_17"], sorted(s["met_at_17"]))
    # 15. both orders of read and fill: a master fill directly behind a master fill — the state's device copies flip —, and one
    # directly behind a read of the state, which fetched it: the fill uploads it again.  Behind a round trip and behind a fill that
    # test_gpu_post_fuzz.py reads the state after (post_walk.peeks)
    assert s["fill_behind_fill"] and s["fill_behind_read"] >= {"roundtrip", "bus"}, s["fill_behind_read"]
    # 16. three refused fills with a meter on
    assert s["refused_with_a_meter"] >= 3


MIRRORS = ("multiband", "limiter", "resampler", "pcm")           # the stages whose state is an S2rMirror that this survey follows
TWO_32 = 1 << 32


def _count(L, M, ph, n):
    """s2r.h, the resampler's step 1: the output frames of a call of n frames at position ph"""
    return 0 if n * L <= ph else -((ph - n * L) // M)


def output_survey(seeds):
    """the stages of OUTPUT_KINDS on the books alone — which is on when, ph, t and the pinned samples' capacity as S2rPostChain keeps
    them, no arithmetic on samples — -> what conditions 17 to 23 ask about"""
    s = dict(kinds=set(), ran=dict(B=set(), lmt=set(), bits=set(), dither=set(), K=set(), detector=set()), first={}, not_first=set(), held_past=[],
             multiband_under=set(), pcm_behind=set(), zero_then_frames=False, big=set(), counts=set(), regrowth=False, another_T=False,
             at_ph={"roundtrip": 0, "handover": 0}, pcm_frames=set(), wrap=False, pcm_carried={"roundtrip": 0, "handover": 0}, pcm_reset=False,
             pcm_another_K=False, another_B=False, params_between=False, multiband_frames=set(), multiband_carried={"roundtrip": 0, "handover": 0},
             tp_short=set(), tp_ceiling=False, switched=set(), tp_loudness_pcm=False, sat={m: set() for m in MIRRORS}, refused=0,
             behind_fill={m: False for m in MIRRORS}, behind_read={m: set() for m in MIRRORS})
    for seed in seeds:
        setup, steps = walk(seed)
        mf = setup["max_frames"]
        loud = spec = False
        mb = lim = res = pcm = None                              # the books: dicts, None while the stage is off
        true_peak, cap = False, 0                                # the walk's detector; the frames the handle's pinned PCM samples hold
        last = {m: None for m in MIRRORS}                        # what each mirror met last: a master "fill", the kind of step that read it, or None
        sat = {m: set() for m in MIRRORS}                        # the fills each stage has sat through since the last master fill that ran it
        on = lambda: dict(multiband=mb, limiter=lim, resampler=res, pcm=pcm)

        def held_past(seed, k):
            """the PCM samples are read here (tests/test_gpu_post_fuzz.py reads them behind every fill, a refused one too): noted where
            they are more frames than max_frames and than the converter that is set NOW makes of max_frames — the samples of a fill
            behind a converter of a ratio above 1 that has been cleared or replaced by a smaller one since"""
            now = mf if res is None else max(mf, -((-mf * res["L"]) // res["M"]) + 1)
            if pcm is not None and pcm.get("frames", 0) > now:
                s["held_past"].append((seed, k))
        s["kinds"] |= {a["kind"] for a in steps}
        for k, a in pw.expanded(steps):                          # (a pause of the meters as the clears and sets it stands for)
            kind = a["kind"]
            if kind in ("loudness_set", "loudness_clear"):
                loud = kind == "loudness_set"
            elif kind in ("spectrum_set", "spectrum_clear"):
                spec = kind == "spectrum_set"
            elif kind == "multiband_set":
                assert a["replaces"] == (mb is not None) and len(a["bands"]) == a["B"], seed
                s["another_B"] |= mb is not None and mb["ran"] > 0 and mb["B"] != a["B"]
                mb, last["multiband"], sat["multiband"] = dict(B=a["B"], ran=0, params=False), None, set()
            elif kind == "multiband_params":
                assert mb is not None and a["B"] == mb["B"], seed
                mb["params"] = mb["ran"] > 0
            elif kind == "multiband_reset":
                assert mb is not None, seed
                mb.update(ran=0, params=False)
                last["multiband"] = None
            elif kind == "multiband_clear":
                assert mb is not None, seed
                mb = None
            elif kind in ("limiter_set", "limiter_reset"):       # (another lookahead or hold: the state resets)
                lim, last["limiter"], sat["limiter"] = dict(tp=true_peak, ran=0, ceiling=False), None, set()
            elif kind == "limiter_clear":
                lim = None
            elif kind == "limiter_ceiling":
                lim["ceiling"] = lim["tp"] and lim["ran"] > 0
            elif kind == "limiter_detector":
                assert a["present"] == (lim is not None) and a["true_peak"] != true_peak, seed
                true_peak = a["true_peak"]
                if lim is not None:
                    if lim["ran"] > 0:
                        s["switched"].add(true_peak)
                    lim, last["limiter"], sat["limiter"] = dict(tp=true_peak, ran=0, ceiling=False), None, set()
            elif kind == "resampler_set":
                assert a["replaces"] == (res is not None) and (a["L"], a["M"], a["T"]) in pw.RESAMPLER_LMT, seed
                s["another_T"] |= res is not None and res["ran"] > 0 and res["T"] != a["T"]
                larger = res is not None and pcm is not None and a["L"] * res["M"] > res["L"] * a["M"]
                res, last["resampler"], sat["resampler"] = dict(L=a["L"], M=a["M"], T=a["T"], ph=0, ran=0, zero=False, larger=larger, between=False), None, set()
            elif kind == "resampler_reset":
                assert res is not None, seed
                res.update(ph=0, ran=0, zero=False)
                last["resampler"] = None
            elif kind == "resampler_clear":
                assert res is not None, seed
                res = None
            elif kind == "pcm_set":
                assert a["replaces"] == (pcm is not None) and a["K"] in pw.PCM_TAPS, seed
                s["pcm_another_K"] |= pcm is not None and pcm["ran"] > 0 and pcm["K"] != a["K"]
                pcm, last["pcm"], sat["pcm"] = dict(K=a["K"], bits=a["bits"], dither=a["dither"], t=0, ran=0, frames=0), None, set()
            elif kind == "pcm_reset":
                assert pcm is not None, seed
                s["pcm_reset"] |= pcm["ran"] > 0
                pcm.update(t=0, ran=0, frames=0)
                last["pcm"] = None
            elif kind == "pcm_clear":
                assert pcm is not None, seed
                pcm = None
                if res is not None:
                    res["zero"] = False
            elif kind == "pcm_wrap":
                assert pcm is not None and a["t"] == pw.PCM_T_WRAP, seed
                pcm["t"], last["pcm"] = a["t"], None
            elif kind == "refused_fill":
                s["refused"] += any(v is not None for v in (mb, res, pcm)) or (lim is not None and lim["tp"])
                held_past(seed, k)
            elif kind in ("roundtrip", "handover"):
                if res is not None and res["ph"] != 0:
                    s["at_ph"][kind] += 1
                if pcm is not None and pcm["ran"] > 0 and pcm["K"] >= 5:
                    s["pcm_carried"][kind] += 1
                if mb is not None and mb["ran"] > 0:
                    s["multiband_carried"][kind] += 1
                for m, book in on().items():
                    if book is not None:
                        last[m] = kind
                if kind == "handover":
                    cap = 0                                      # a fresh handle: its first master fill with the stage allocates
                    if pcm is not None:
                        pcm["frames"] = 0                        # ... and it holds no samples
            elif kind == "fill" and a["fill"] in ("bus", "panned"):
                held_past(seed, k)
                for m, book in on().items():
                    if book is not None and book["ran"] > 0:
                        sat[m].add(a["fill"])
                    if book is not None and pw.peeks(k):
                        last[m] = a["fill"]
                if res is not None and res["larger"]:
                    res["between"] = True
            elif kind == "fill":
                n = a["frames"]
                behind = [name for name, there in zip(pw.MASTER_STAGES, (loud, spec, res is not None, pcm is not None)) if there]
                if behind:                                       # the first kernel behind the master section copies the master out
                    s["first"][behind[0]] = s["first"].get(behind[0], 0) + 1
                    s["not_first"] |= set(behind[1:])
                for m, book in on().items():
                    if book is None:
                        continue
                    if last[m] == "fill":
                        s["behind_fill"][m] = True
                    elif last[m] is not None:
                        s["behind_read"][m].add(last[m])
                    if m != "limiter" or book["tp"]:
                        s["sat"][m] |= sat[m]
                    last[m], sat[m] = "fill", set()
                if mb is not None:
                    s["ran"]["B"].add(mb["B"])
                    s["multiband_under"].add("off" if lim is None else "true" if lim["tp"] else "sample")
                    s["params_between"] |= mb["params"]
                    s["multiband_frames"].add(n)
                    mb["ran"], mb["params"] = mb["ran"] + n, False
                if lim is not None:
                    s["ran"]["detector"].add(lim["tp"])
                    if lim["tp"] and lim["ran"] > 0:
                        s["tp_short"] |= {name for name, there in (("under 8", n < 8), ("8 to 15", 8 <= n < 16)) if there}
                        s["tp_ceiling"] |= lim["ceiling"]
                    s["tp_loudness_pcm"] |= lim["tp"] and loud and pcm is not None
                    lim["ran"], lim["ceiling"] = lim["ran"] + n, False
                made = n
                if res is not None:
                    made = _count(res["L"], res["M"], res["ph"], n)
                    assert made <= -((-n * res["L"]) // res["M"]) + 1, seed
                    s["ran"]["lmt"].add((res["L"], res["M"], res["T"]))
                    s["big"] |= {"resampler"} if n > 1024 else set()
                    s["counts"] |= {name for name, there in (("over 64", made > 64), ("under 64", 0 < made < 64)) if there}
                    if pcm is not None:
                        s["zero_then_frames"] |= res["zero"] and made > 0
                        res["zero"] = res["zero"] or made == 0
                    else:
                        res["zero"] = False                      # (the same pair of stages: a PCM stage set later has not met the empty call)
                    res["ph"] += made * res["M"] - n * res["L"]
                    assert 0 <= res["ph"] < res["M"], seed
                    res["ran"] += n
                if pcm is not None:
                    need = mf if res is None else -((-mf * res["L"]) // res["M"]) + 1     # S2R_RESAMPLER_MAX_OUT
                    if cap < need:                               # (a regrowth where the handle held pinned samples already)
                        s["regrowth"] |= cap > 0 and res is not None and res["larger"] and res["between"]
                        cap = need
                    s["pcm_behind"].add(res is not None)
                    pcm["frames"] = made
                    if made:
                        s["ran"]["bits"].add(pcm["bits"]); s["ran"]["dither"].add(pcm["dither"]); s["ran"]["K"].add(pcm["K"])
                        s["pcm_frames"] |= {name for name, there in (("one", made == 1), ("under K", made < pcm["K"]), ("three tiles", made >= 257)) if there}
                        s["wrap"] |= pcm["t"] + made > TWO_32
                        pcm["t"], pcm["ran"] = (pcm["t"] + made) % TWO_32, pcm["ran"] + made
                if res is not None:
                    res["larger"] = res["between"] = False
    return s


def test_the_default_walks_cover_the_output_stages():
    """the conditions on the third generator (post_walk._splice_outputs), asserted the way the others are: its weights are chosen so
    that they hold over the default seeds"""
    s = output_survey(DEFAULTS)
    # 17. every kind; every band count, (L, M, T), bits, dither kind, tap count and both detectors run in a master fill
    assert s["kinds"] >= set(pw.OUTPUT_KINDS), set(pw.OUTPUT_KINDS) - s["kinds"]
    assert s["ran"]["B"] == {1, 2, 3, 4} and s["ran"]["lmt"] == set(pw.RESAMPLER_LMT), (s["ran"]["B"], set(pw.RESAMPLER_LMT) - s["ran"]["lmt"])
    assert s["ran"]["bits"] == set(pw.PCM_BITS) and s["ran"]["dither"] == set(pw.PCM_DITHERS) and s["ran"]["K"] == set(pw.PCM_TAPS), s["ran"]
    assert s["ran"]["detector"] == {False, True}
    # 18. each of the four kernels behind the limiter copies the master out in some fill and does not in another; the multiband stage
    # with the limiter off and under either detector; the PCM stage behind a resampler and without one
    assert set(s["first"]) == set(pw.MASTER_STAGES) and min(s["first"].values()) >= 2, s["first"]      # each in two fills at the least
    assert s["not_first"] == set(pw.MASTER_STAGES[1:]), s["not_first"]       # (the loudness kernel is the first whenever it runs)
    assert s["multiband_under"] == {"off", "sample", "true"} and s["pcm_behind"] == {False, True}, (s["multiband_under"], s["pcm_behind"])
    # 19. the resampler: a call that makes no frame with the PCM stage on and a later one on the same pair that does; more than 1024
    # frames; more and fewer than 64 outputs; a regrowth of the pinned samples with a bus fill or a panned fill in front of it;
    # another T; a round trip and a handover at ph != 0
    assert s["zero_then_frames"] and "resampler" in s["big"] and s["counts"] == {"over 64", "under 64"}, (s["zero_then_frames"], s["big"], s["counts"])
    assert s["regrowth"] and s["another_T"] and all(s["at_ph"].values()), (s["regrowth"], s["another_T"], s["at_ph"])
    # 20. the PCM stage: calls of 1 frame, of fewer than K and of three tiles; t across 2^32; a round trip and a handover in mid-stream
    # with K >= 5; a reset, and a set again with another K
    assert s["pcm_frames"] == {"one", "under K", "three tiles"} and s["wrap"], (s["pcm_frames"], s["wrap"])
    assert all(s["pcm_carried"].values()) and s["pcm_reset"] and s["pcm_another_K"], (s["pcm_carried"], s["pcm_reset"], s["pcm_another_K"])
    # 21. the multiband stage: another B in mid-state; new parameters between two fills; calls of 1 and 2 frames and of more than
    # 1024; a round trip and a handover
    assert s["another_B"] and s["params_between"] and s["multiband_frames"] >= {1, 2} and max(s["multiband_frames"]) > 1024
    assert all(s["multiband_carried"].values()), s["multiband_carried"]
    # 22. the true-peak limiter: calls of fewer than 8 and of 8 to 15 frames on a state that has run; a ceiling move that keeps it; the
    # detector switched in either direction on a limiter that has run; the loudness meter and the PCM stage behind it in one fill
    assert s["tp_short"] == {"under 8", "8 to 15"} and s["tp_ceiling"] and s["switched"] == {False, True} and s["tp_loudness_pcm"], (
        s["tp_short"], s["tp_ceiling"], s["switched"], s["tp_loudness_pcm"])
    # 23. each stage sits through a bus fill and a panned fill between two master fills; three refused fills with one of them on; a
    # master fill directly behind a master fill and directly behind a read of the state, with each mirror present (condition 15)
    assert all(v == {"bus", "panned"} for v in s["sat"].values()) and s["refused"] >= 3, (s["sat"], s["refused"])
    assert all(s["behind_fill"].values()) and all(v >= {"roundtrip", "bus"} for v in s["behind_read"].values()), (s["behind_fill"], s["behind_read"])


def test_the_regression_seeds_read_pcm_samples_held_past_their_converter():
    """post_walk.REGRESSION_SEEDS: the walks that found the fault in Synth.pcm, which sized its buffer by the converter that is set now.
    On the books: a master fill behind a converter of a ratio above 1 leaves the PCM stage more than max_frames samples; the converter
    is then cleared, or replaced by one of a smaller ratio, and the samples, still held (s2r.h), are read behind a bus fill, a panned
    fill or a refused fill before the next master fill.  No default seed does that; these run beside them on the device, and through
    the model alone here"""
    held = output_survey(pw.REGRESSION_SEEDS)["held_past"]
    assert {seed for seed, _ in held} == set(pw.REGRESSION_SEEDS) and (500030, 33) in held, held
    assert not output_survey(DEFAULTS)["held_past"]
    for seed in pw.REGRESSION_SEEDS:
        chain, fills = run_on_the_model(*walk(seed), seed)
        _check_model_run(chain, fills, "seed %d" % seed)


def test_the_subset_walk_makes_96_calls_over_the_32_subsets():
    setup, steps = pw.subset_walk()
    on, seen, calls = {st: set() for st in INSERTS}, [], 0
    for a in steps:
        if a["kind"] == "set" and a["stage"] in INSERTS:
            on[a["stage"]].add(a["bus"])
        elif a["kind"] == "clear":
            on[a["stage"]].discard(a["bus"])
        elif a["kind"] == "fill":
            calls += 1
            now = frozenset(st for st in INSERTS if on[st])
            if not seen or seen[-1] != now:
                seen.append(now)
            assert (a["n_buses"], a["frames"]) == (3, 33)
    assert calls == 96 and len(seen) == 32 and set(seen) == set(_subsets(INSERTS))
    assert all(len(p ^ q) == 1 for p, q in zip(seen, seen[1:]))  # Gray-code order: one insert set or cleared per step
    assert [a["fill"] for a in steps if a["kind"] == "fill"] == ["bus", "master_stems", "master"] * 32
    # the flanger: on two of the three buses, one with H = 33, the other with a feedback and a cross, one beside the drive, one beside the room
    fl = {a["bus"]: a["shape"] for a in steps if a["kind"] == "set" and a["stage"] == "flanger"}
    beside = {st: {a["bus"] for a in steps if a["kind"] == "set" and a["stage"] == st} for st in ("drive", "room")}
    assert len(fl) == 2 and sorted(q["H"] == 33 for q in fl.values()) == [False, True]
    assert any(q["H"] != 33 and q["feedback"] != 0.0 and q["cross"] != 0.0 for q in fl.values())
    assert set(fl) & beside["drive"] and set(fl) & beside["room"]


def _dry(rng, nb, n):
    """in place of the twin's buses: seeded float32 noise whose peak is the twin's"""
    return (rng.uniform(-1.0, 1.0, (nb, n, 2)) * TWIN_PEAK).astype(F)


def run_on_the_model(setup, steps, seed):
    """a walk through Chain alone -> per fill (step index, action, what Chain.expect returns)"""
    chain, rng, out = Chain(), np.random.RandomState(seed ^ 0x5EED), []
    for k, a in enumerate(steps):
        if a["kind"] == "handover":
            chain.handed_over()                                  # what post_walk.handover leaves on the model
        elif a["kind"] != "fill":
            chain.apply(a)
        else:
            x = _dry(rng, a["n_buses"], a["frames"]) if a["fill"] != "panned" else (rng.uniform(-1.0, 1.0, (a["frames"], 2)) * TWIN_PEAK).astype(F)
            out.append((k, a, chain.expect(x, a, "seed %d, step %d" % (seed, k))))
            # the states of the stages behind the master section behind every fill, not only of those that live to the end of the walk
            for name, v in chain.meter_states().items():
                assert np.isfinite(v).all(), "seed %d, step %d %r: the state of %s is not finite" % (seed, k, a, name)
    return chain, out


def _check_model_run(chain, fills, what):
    limit = 2.0 ** 20                                            # S2R_LIMITER_CEILING_LOG2: the limiter's largest ceiling
    for k, a, e in fills:
        for name in ("panned", "buses", "stems", "master", "peaks", "energies"):
            if name in e:
                assert np.isfinite(e[name]).all(), "%s, step %d %r: %s is not finite" % (what, k, a, name)
                if name != "energies":
                    assert float(np.abs(e[name]).max()) <= limit, "%s, step %d %r: %s reaches %g" % (what, k, a, name, float(np.abs(e[name]).max()))
        for st, bus, changed, excused in e["trace"]:
            assert changed or excused, "%s, step %d %r: the %s on bus %d changes no bit of its input" % (what, k, a, st, bus)
        for name in ("loudness rows", "true peak", "true peak held", "spectrum rows", "multiband meters", "resampled"):
            if name in e and not isinstance(e[name], int):
                assert np.isfinite(e[name]).all(), "%s, step %d %r: the %s are not finite" % (what, k, a, name)
        # as tests/test_gpu_post_fuzz.py asks of every limited fill: Chain.expect lowers the ceiling where a master would stay under it
        assert "gain" not in e or (e["gain"] < 1.0).any() or e["idle"] or e["limiter in"] <= 2.0 ** -19, "%s, step %d %r: the limiter does not work" % (what, k, a)
    # a converter that reads silence tests nothing: of every one that ran, every programme that sounded has a bit set in some output
    for serial, (sounded, made) in chain.resampled.items():
        assert sounded <= made, "%s: the %dth converter to start makes +0.0 of programmes %s" % (what, serial, sorted(sounded - made))
    # a meter that reads silence throughout tests nothing: of every meter, from the set or reset that started it, every programme that
    # sounded (above 2^-10) in the frames a completed row is taken over has a row entry above 0.0
    sounded, positive = {}, {}
    for k, a, e in fills:
        for m in e.get("meters", ()):
            key = (m["name"],) + m["instance"]
            sounded.setdefault(key, set()).update(m["sounding"])
            positive.setdefault(key, set()).update(m["positive"])
    for key, programmes in sounded.items():
        assert programmes <= positive[key], "%s: the %s meter (the %dth to start) reads silence on programmes %s" % (
            what, key[0], key[1], sorted(programmes - positive[key]))
    for name, v in chain.states().items():
        assert np.isfinite(v).all(), "%s: the state of %s" % (what, name)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_model_alone_is_well_behaved(seed):
    """every expected buffer is finite and within the limiter's largest ceiling, and every stage that runs changes a bit of its input or
    is in a case its own file documents as an identity"""
    setup, steps = walk(seed)
    chain, fills = run_on_the_model(setup, steps, seed)
    assert len(fills) >= 12
    _check_model_run(chain, fills, "seed %d" % seed)


def test_the_model_alone_is_well_behaved_over_the_subset_walk():
    setup, steps = pw.subset_walk()
    chain, fills = run_on_the_model(setup, steps, 1)
    _check_model_run(chain, fills, "the subset walk")
    assert any(len(e["trace"]) == 12 for _, _, e in fills)       # all five inserts on two buses each, the chorus and the reverb
    assert chain.recursion[1] == 2 * 48 * 33 and chain.recursion[0] >= chain.recursion[1] / 10.0, chain.recursion
    assert all((e["gain"] < 1.0).any() for _, a, e in fills if a["fill"] == "master")
    # both meters from the start to the end: 64 master fills of 33 frames are 2112 frames, 124 hops of 17 and 16 of 128
    metered = [e for _, a, e in fills if a["fill"] != "bus"]
    assert len(metered) == 64 and all([m["name"] for m in e["meters"]] == ["loudness", "spectrum"] for e in metered)
    assert chain.loud.made == 2112 // 17 and chain.spec.made == 2112 // 128 and (chain.loud.pos, chain.spec.pos) == (2112 % 17, 2112 % 128)
    assert all(e["loudness hops"] == min(32, (33 * (i + 1)) // 17) for i, e in enumerate(metered))
    assert (chain.loud.rows[:, :6] > 0.0).all() and (chain.loud.rows[:, 16:] > 0.0).all() and (chain.spec.rows[:, [0, 1, 2, 8]] > 0.0).any(axis=2).all()


def test_the_flangers_recursion_shows_over_the_default_walks():
    """FlangerModel carries beside each flanger the same flanger at feedback = cross = 0, fed the same input: over the default seeds the
    flangers with a feedback or a cross differ from that twin on bits in at least a tenth of the frames they ran — the per-stage
    file's threshold (FlangerModel.busy), over the sweep as a whole: a walk's flanger may live for two short calls"""
    differs = frames = 0
    for seed in DEFAULTS:
        chain, _ = run_on_the_model(*walk(seed), seed)
        differs, frames = differs + chain.recursion[0], frames + chain.recursion[1]
    assert frames > 0 and differs >= frames / 10.0, "the recursion shows in %d of %d frames" % (differs, frames)


def test_the_output_stages_work_over_the_default_walks():
    """a stage that reads silence or does nothing tests nothing.  Summed over the default seeds, on the model alone, as the flanger's
    recursion is: every band of the multiband stage takes both branches of the ballistics and has a least gain below 1
    (test_gpu_multiband.Mb.both_branches, per band index); under the true-peak detector d differs on bits from the sample magnitude in
    a tenth of the frames and a tenth are limited (test_gpu_limiter_tp.LimTp.interpolated); a tenth of the samples the PCM stage is
    fed do not clip, and both rails do; and with taps the integers differ from those of the same stage without, fed the same input,
    in a tenth of the frames"""
    B = 4
    n_att, n_rel, least = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.full(B, np.inf)
    tp, shaped, unclipped, rails = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), set()
    for seed in DEFAULTS:
        chain, _ = run_on_the_model(*walk(seed), seed)
        for mb in chain.mbs:
            n_att[:mb.B] += mb.n_att; n_rel[:mb.B] += mb.n_rel
            least[:mb.B] = np.minimum(least[:mb.B], mb.least)
        tp += chain.true_peak_frames; shaped += chain.shaped; unclipped += chain.unclipped
        rails |= chain.rails
    print("multiband: attack frames %s, release frames %s, least gains %s; true peak: %s of %d frames limited, %s interpolated; PCM: %s of %s frames "
          "shaped, %s of %s samples unclipped, rails %s" % (n_att, n_rel, least, tp[0], tp[2], tp[1], shaped[0], shaped[1], unclipped[0], unclipped[1], sorted(rails)))
    assert (n_att > 0).all() and (n_rel > 0).all() and (least < 1.0).all(), (n_att, n_rel, least)
    assert tp[2] > 0 and tp[0] >= tp[2] / 10.0 and tp[1] >= tp[2] / 10.0, tp
    assert shaped[1] > 0 and shaped[0] >= shaped[1] / 10.0, shaped
    assert unclipped[1] > 0 and unclipped[0] >= unclipped[1] / 10.0 and rails == {"low", "high"}, (unclipped, rails)


def test_the_master_subset_walk_makes_48_master_fills_over_the_16_subsets():
    setup, steps = pw.master_subset_walk()
    assert setup == dict(max_frames=300, timing=False)
    sets = {st + "_set": st for st in pw.MASTER_STAGES}
    clears = {st + "_clear": st for st in pw.MASTER_STAGES}
    on, seen, fills, limiter, detector, mb = set(), [], [], False, False, False
    for a in steps:
        kind = a["kind"]
        if kind in sets:
            assert sets[kind] not in on
            on.add(sets[kind])
        elif kind in clears:
            on.remove(clears[kind])
        elif kind in ("limiter_set", "limiter_clear"):
            limiter = kind == "limiter_set"
        elif kind == "limiter_detector":
            assert a["present"] == limiter
            detector = a["true_peak"]
        elif kind in ("multiband_set", "multiband_clear"):
            mb = kind == "multiband_set"
            assert not mb or a["B"] == 3
        elif kind == "fill":
            now = frozenset(on)
            if not seen or seen[-1] != now:
                seen.append(now)
            assert a["n_buses"] == 3 and a["fill"] in ("master", "master_stems")
            fills.append((a["frames"], a["fill"] == "master_stems", mb, "off" if not limiter else "true" if detector else "sample"))
    assert len(fills) == 48 and len(seen) == 16 and set(seen) == set(_subsets(pw.MASTER_STAGES))
    assert all(len(p ^ q) == 1 for p, q in zip(seen, seen[1:]))  # Gray-code order: one stage set or cleared per step
    assert [f[0] for f in fills] == list(pw.MASTER_SUBSET_FRAMES) * 6 and [f[3] for f in fills] == ["off", "sample", "true"] * 16
    # with and without stems, with and without the multiband stage, under every state of the limiter
    assert {f[1:] for f in fills} == {(st, m, lim) for st in (False, True) for m in (False, True) for lim in ("off", "sample", "true")}
    faders = [a["level"] for a in steps if a["kind"] == "fader"]
    assert faders == list(pw.MASTER_SUBSET_FADERS) * 8            # from subset to subset, each move snapped in front of the subset's fills
    assert all(b["kind"] == "snap" for a, b in zip(steps, steps[1:]) if a["kind"] == "fader")
    res = [a for a in steps if a["kind"] == "resampler_set"]
    pcm = [a for a in steps if a["kind"] == "pcm_set"]
    assert all((a["L"], a["M"], a["T"]) == (147, 160, 48) for a in res) and all((a["bits"], a["dither"], a["K"]) == (16, "tpdf", 9) for a in pcm)
    assert any(a["kind"] == "set" and a["stage"] == "eq" for a in steps) and any(a["kind"] == "set" and a["stage"] == "room" for a in steps)
    assert not any(a["kind"] == "clear" for a in steps)


def test_the_model_alone_is_well_behaved_over_the_master_subset_walk():
    """... and on the model: in the subsets at the low setting of the master fader, 0.125, the master programme stays inside full scale —
    three buses at TWIN_PEAK sum to 0.82 at the most, and what the converter's and the limiter's histories carry in from the subset
    before is under the limiter's ceiling — and the PCM stage clips nothing on programme 8: all 12 of those fills with the stage on.
    Of the 12 at 1, the master clips in the two that have both the limiter and the multiband compressor off, fills 24 and 36, of 127
    and 9 frames.  The others are not asserted to clip, because they need not: under the limiter the master is held to a ceiling of
    half the quietest master's peak, which lies inside full scale (Chain.ceiling) — what still clips there is the loud fill before,
    carried in by the limiter's delay and the converter's histories —, and the two with the compressor alone, fills 30 and 42, are
    brought inside full scale by thresholds 24 and 14 dB below TWIN_PEAK and clip nothing, which is asserted"""
    setup, steps = pw.master_subset_walk()
    chain, fills = run_on_the_model(setup, steps, 2)
    _check_model_run(chain, fills, "the master subset walk")
    assert len(fills) == 48
    limiter, mb, low, clipped, kept, compressed = False, False, None, {}, {}, {}
    runs = enumerate(fills)
    for a in steps:
        if a["kind"] in ("limiter_set", "limiter_clear"):
            limiter = a["kind"] == "limiter_set"
        elif a["kind"] in ("multiband_set", "multiband_clear"):
            mb = a["kind"] == "multiband_set"
        elif a["kind"] == "fader":
            low = a["level"] == pw.MASTER_SUBSET_FADERS[1]
        elif a["kind"] == "fill":
            f, (_, _, e) = next(runs)
            if "pcm clips" in e:
                (kept if low else {} if limiter else compressed if mb else clipped)[f] = int(e["pcm clips"][2 * 8:].sum())
                assert e["count"] < 64 or e["pcm clips"][2 * 2:2 * 3].all(), "bus 2, dry at TWIN_PEAK, does not clip in 64 frames"
    assert len(kept) == 12 and not any(kept.values()), kept
    assert sorted(clipped) == [24, 36] and all(clipped.values()), clipped
    assert sorted(compressed) == [30, 42] and not any(compressed.values()), compressed
    # the multiband stage and the true-peak detector work, the converter makes frames, and the shaper shows
    assert len(chain.mbs) == 12                                  # (set afresh every fourth fill)
    n_att, n_rel, least = sum(mb.n_att for mb in chain.mbs), sum(mb.n_rel for mb in chain.mbs), np.minimum.reduce([mb.least for mb in chain.mbs])
    assert (n_att > 0).all() and (n_rel > 0).all() and (least < 1.0).all(), (n_att, n_rel, least)
    assert chain.true_peak_frames[2] == sum(pw.MASTER_SUBSET_FRAMES) * 2 and chain.true_peak_frames[1] >= chain.true_peak_frames[2] / 10.0
    assert chain.shaped[1] > 0 and chain.shaped[0] >= chain.shaped[1] / 10.0, chain.shaped
    assert len(chain.resampled) == 1 and chain.resampled[1][1] == {0, 1, 2, 8}       # one converter, from the fifth subset to the twelfth
