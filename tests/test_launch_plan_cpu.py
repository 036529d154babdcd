"""The launch planner (csrc/brotli_launch_plan.h) against plans RECORDED from real launches: tests/golden/launch_plans.json holds, for
batches that take every branch of submit() and of the later passes, what the library launched on an MI355X before the planner was split
from submit() -- grid, waves, arena, blocks per CU, gang word, order, and how many descriptors carried ENGINE_ONLY, DEFER and NO_SPILL --
beside what the planner is given: the device's facts, per_cu_cap, the compressed sizes and the probe's kinds.  No GPU is needed: the
planner is a pure function, reached through BrotliAmdDebugPlanLaunch / BrotliAmdDebugPlanLaterPass."""
import ctypes
import json
import os

import pytest

from conftest import ROOT, load_pkg

u32, i32 = ctypes.c_uint32, ctypes.c_int32


class PlanDevice(ctypes.Structure):  # BrotliAmdPlanDevice
    _fields_ = [(k, u32) for k in ("cus", "lds_per_cu", "block_max", "lds_fixed", "lds_helper4", "lds_helper8", "lds_helper16", "lds_arena",
                                   "max_arena", "grid_max", "retry_grid_max", "auto_arena", "engine_ok")]


class PlanKnobs(ctypes.Structure):  # BrotliAmdPlanKnobs
    _fields_ = [("max_blocks_per_cu", u32), ("min_small_arena", u32), ("no_scan", u32), ("no_engine_queue", u32), ("engine_queue_max", u32),
                ("no_record_blocks", u32), ("no_order", u32), ("gang", i32), ("pool", i32), ("gang_no_helpers", u32), ("debug_probe", u32)]


class LaunchPlan(ctypes.Structure):  # BrotliAmdLaunchPlan
    _fields_ = [(k, u32) for k in ("grid", "waves", "arena", "cur_per_cu", "gang", "ordered", "want_probe", "engine_queue", "no_spill")]


class LaterPass(ctypes.Structure):  # BrotliAmdLaterPass
    _fields_ = [(k, u32) for k in ("level", "arena", "grid_max", "waves", "last")]


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    L = pkg.load_library()
    L.BrotliAmdDebugPlanLaunch.argtypes = [ctypes.POINTER(PlanDevice), ctypes.POINTER(PlanKnobs), u32, u32, ctypes.POINTER(ctypes.c_size_t),
                                           ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(LaunchPlan)]
    L.BrotliAmdDebugPlanLaterPass.argtypes = [ctypes.POINTER(PlanDevice), ctypes.POINTER(PlanKnobs), u32, u32, u32, u32, ctypes.c_int,
                                              ctypes.POINTER(LaterPass)]
    return L


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")))


def unrle(runs):
    return [v for v, count in runs for _ in range(count)]


def plan_launch(lib, dev, knobs, per_cu_cap, sizes, kinds):
    plan = LaunchPlan()
    a_sizes = (ctypes.c_size_t * len(sizes))(*sizes)
    a_kinds = (ctypes.c_uint8 * len(kinds))(*kinds) if kinds is not None else None
    assert lib.BrotliAmdDebugPlanLaunch(ctypes.byref(dev), ctypes.byref(knobs), per_cu_cap, len(sizes), a_sizes, a_kinds, ctypes.byref(plan)) == 0
    return plan


def shape(plan):
    return {k: getattr(plan, k) for k in ("grid", "waves", "arena", "cur_per_cu", "gang", "ordered")}


def test_the_fixture_takes_every_branch(recorded):
    """what the recording is for: every shape submit() and the later passes can give is in it"""
    launches = [e for c in recorded["cases"] for e in c["events"] if e["ev"] == "launch"]
    later = [e for c in recorded["cases"] for e in c["events"] if e["ev"] == "later"]
    gangs = {e["plan"]["gang"] for e in launches}
    assert {0, 2, 4, 8, 16, 0x108} <= gangs, gangs
    probes = [e for c in recorded["cases"] for e in c["events"] if e["ev"] == "probe"]
    assert {1, 4, 16} <= {e["plan"]["waves"] for e in launches} and 8 in {e["waves"] for e in probes}   # (eight-wave blocks: a probe's own launch)
    assert any(e["kinds"] is not None and e["plan"]["engine_only"] for e in launches)          # probe, then the engine queue
    assert any(e["kinds"] is not None and not e["plan"]["engine_only"] and e["plan"]["waves"] == 4 and e["n"] > 1024 for e in launches)   # record blocks
    assert any(e["kinds"] is None and e["n"] >= 2048 for e in launches)                       # many small streams: no probe
    assert any(e["plan"]["cur_per_cu"] > 8 for e in launches)                                   # one-wave blocks with a small arena
    assert any(not recorded["devices"][e["dev"]]["auto_arena"] for e in launches)
    assert any(e["plan"]["defer"] for e in launches) and any(e["deferred"] for e in later)
    # a later pass at each level: eight one-wave blocks a CU, the configured arena, the largest arena
    devs = recorded["devices"]
    assert any(e["plan"]["waves"] == 1 and not e["deferred"] for e in later)
    assert any(e["plan"]["arena"] == devs[e["dev"]]["lds_arena"] and not e["deferred"] for e in later)
    assert any(e["plan"]["arena"] == devs[e["dev"]]["max_arena"] for e in later)


def test_the_planner_gives_the_recorded_plans(lib, recorded):
    knobs = PlanKnobs(**recorded["knobs"])
    checked = 0
    for case in recorded["cases"]:
        probe = None
        for e in case["events"]:
            where = (case["case"], e)
            if e["ev"] == "probe":
                probe = e
                continue
            dev = PlanDevice(**recorded["devices"][e["dev"]])
            if e["ev"] == "later":
                p = LaterPass()
                assert lib.BrotliAmdDebugPlanLaterPass(ctypes.byref(dev), ctypes.byref(knobs), e["per_cu_cap"], e["level_in"], e["cur_arena"], e["m"],
                                                       e["deferred"], ctypes.byref(p)) == 0
                assert {"grid": min(e["m"], p.grid_max), "arena": p.arena, "waves": p.waves} == e["plan"], where
                checked += 1
                continue
            assert e["ev"] == "launch"
            sizes, want = unrle(e["sizes"]), e["plan"]
            assert len(sizes) == e["n"]
            first = plan_launch(lib, dev, knobs, e["per_cu_cap"], sizes, None)
            if e["kinds"] is None:
                assert not first.want_probe, where
                plan = first
            else:
                # the device was asked (or had been asked about the same descriptors before): the planner wants that, and the shape it gives
                # the probe's own launch is the one the probe had
                assert first.want_probe, where
                if probe is not None and probe["n"] == e["n"]:
                    assert {k: getattr(first, k) for k in ("grid", "waves", "arena")} == {k: probe[k] for k in ("grid", "waves", "arena")}, where
                kinds = unrle(e["kinds"])
                plan = plan_launch(lib, dev, knobs, e["per_cu_cap"], sizes, kinds)
                assert not plan.want_probe, where
            want_shape = {k: want[k] for k in ("grid", "waves", "arena", "cur_per_cu", "gang", "ordered")}
            assert shape(plan) == want_shape, (where, shape(plan))
            engines = sum(1 for k in unrle(e["kinds"]) if k == 7) if plan.engine_queue else 0
            assert (engines, e["n"] - engines if plan.engine_queue else 0) == (want["engine_only"], want["defer"]), where
            assert (e["n"] - e["spill_in_place"] if plan.no_spill else 0) == want["no_spill"], where
            probe = None
            checked += 1
    assert checked >= 30, checked


def test_the_planner_refuses_what_it_cannot_plan(lib):
    dev, knobs, plan = PlanDevice(cus=256), PlanKnobs(), LaunchPlan()
    one = (ctypes.c_size_t * 1)(1000)
    assert lib.BrotliAmdDebugPlanLaunch(ctypes.byref(dev), ctypes.byref(knobs), 14, 0, one, None, ctypes.byref(plan)) == -1
    assert lib.BrotliAmdDebugPlanLaunch(ctypes.byref(dev), ctypes.byref(knobs), 14, 1, None, None, ctypes.byref(plan)) == -1
    assert lib.BrotliAmdDebugPlanLaunch(None, ctypes.byref(knobs), 14, 1, one, None, ctypes.byref(plan)) == -1
    assert lib.BrotliAmdDebugPlanLaunch(ctypes.byref(PlanDevice()), ctypes.byref(knobs), 14, 1, one, None, ctypes.byref(plan)) == -1
