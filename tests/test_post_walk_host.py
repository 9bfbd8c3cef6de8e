"""What the seeded walks of tests/post_walk.py cover, and that the chain's host model alone is well behaved over them — on the CPU, over
the default seeds of tests/test_gpu_post_fuzz.py.  The coverage conditions are conditions on the inputs: the generator's weights and the
default seed count are chosen so that they hold, and this file asserts them."""
import itertools
import os

import numpy as np
import pytest

import post_walk as pw
from post_walk import FILLS, INSERTS, STAGES, STEMS, TWIN_PEAK, Chain, walk

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
        assert 20 <= len(steps) <= 30 and sum(a["kind"] == "fill" for a in steps) >= 12, seed
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
            chain.lim_meters = None                              # what post_walk.handover leaves of it on the model
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


def test_the_flangers_recursion_shows_over_the_default_walks():
    """FlangerModel carries beside each flanger the same flanger at feedback = cross = 0, fed the same input: over the default seeds the
    flangers with a feedback or a cross differ from that twin on bits in at least a tenth of the frames they ran — the per-stage
    file's threshold (FlangerModel.busy), over the sweep as a whole: a walk's flanger may live for two short calls"""
    differs = frames = 0
    for seed in DEFAULTS:
        chain, _ = run_on_the_model(*walk(seed), seed)
        differs, frames = differs + chain.recursion[0], frames + chain.recursion[1]
    assert frames > 0 and differs >= frames / 10.0, "the recursion shows in %d of %d frames" % (differs, frames)
