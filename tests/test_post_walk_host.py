"""What the seeded walks of tests/post_walk.py cover, and that the chain's host model alone is well behaved over them — on the CPU, over
the default seeds of tests/test_gpu_post_fuzz.py.  The coverage conditions are conditions on the inputs: the generator's weights and the
default seed count are chosen so that they hold, and this file asserts them."""
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
    assert pw.subset_walk() == pw.subset_walk()


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
        for k, a in enumerate(steps):
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
        for name in ("loudness rows", "true peak", "true peak held", "spectrum rows"):
            if name in e:
                assert np.isfinite(e[name]).all(), "%s, step %d %r: the %s are not finite" % (what, k, a, name)
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
