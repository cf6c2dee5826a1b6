"""The table of the stepper's optional terms without a GPU: ``term_plan`` over every on/off combination of the ten optional weights
against the two orders and the two lists written out below (taken from the stepper before the table existed, not from the code under
test), the key order and the refusals of ``merge_weights``, the default gates of ``select_tolerances``, and which error comes first
when a constructor call is wrong twice (stand-ins for the hand and the objects: the checks come before the device)."""
import itertools

import numpy as np
import pytest
import torch

import _arm_oracle as ao
import _reach_oracle as ro

FIXED = ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints")
DECLARATION = ("E_prior", "E_wall", "E_scene", "E_approach", "E_pregrasp", "E_squeeze", "E_reach", "E_arm", "E_track", "E_lift")
LAUNCH = ("tabletop", "scene", "approach", "pregrasp", "lift", "squeeze", "reach", "track", "arm")
KEY_OF = {"E_prior": "tabletop", "E_wall": "tabletop", "E_scene": "scene", "E_approach": "approach", "E_pregrasp": "pregrasp",
          "E_squeeze": "squeeze", "E_reach": "reach", "E_arm": "arm", "E_track": "track", "E_lift": "lift"}
NEEDS_SAMPLES = ("tabletop", "scene", "approach", "pregrasp", "lift")
G_THETA = ("pregrasp", "squeeze")
GATED = ("E_scene", "E_approach", "E_pregrasp", "E_arm", "E_lift")
MERGED_KEYS = list(FIXED) + ["E_lift", "E_track", "E_arm", "E_reach", "E_squeeze", "E_prior", "E_wall", "E_scene", "E_approach",
                             "E_pregrasp"]


def test_term_plan_over_every_combination():
    from graspqp_amd.stepper import merge_weights, term_plan

    n_seen = 0
    for bits in itertools.product((0.0, 1.5), repeat=len(DECLARATION)):
        w = dict(zip(DECLARATION, bits))
        on_names = [k for k in DECLARATION if w[k] > 0]
        if "E_prior" in on_names or "E_wall" in on_names:  # either weight switches tabletop on, and both rows appear
            on_names = ["E_prior", "E_wall"] + [k for k in on_names if k not in ("E_prior", "E_wall")]
        on_keys = {KEY_OF[k] for k in on_names}
        for weights in (w, merge_weights(w)):  # the bare dict and the merged one the constructor hands over
            plan = term_plan(weights)
            assert plan.term_names == FIXED + tuple(on_names), w
            assert plan.launch == tuple(k for k in LAUNCH if k in on_keys), w
            assert plan.fuse_loop == (len(plan.term_names) == 5), w
            assert plan.needs_samples == any(k in on_keys for k in NEEDS_SAMPLES), w
            assert plan.g_theta == any(k in on_keys for k in G_THETA), w
        n_seen += 1
    assert n_seen == 1024
    assert term_plan({}).term_names == FIXED and term_plan({}).launch == () and term_plan({}).fuse_loop
    assert term_plan({"E_scene": 0.0}).fuse_loop  # weight 0 is off


def test_table_rows_are_plain_data_in_declaration_order():
    from graspqp_amd import stepper as S

    assert tuple(k for t in S.TERMS for k in t.names) == DECLARATION
    assert [t.key for t in S.TERMS] == ["tabletop", "scene", "approach", "pregrasp", "squeeze", "reach", "arm", "track", "lift"]
    assert S.LAUNCH_ORDER == LAUNCH
    assert tuple(k for t in S.TERMS if t.gated for k in t.names) == GATED
    assert {t.key: t.total for t in S.TERMS} == dict({k: "gq_scene_total" for k in LAUNCH}, tabletop="gq_tabletop_total")
    for t in S.TERMS:  # a term's three pieces stand under its key
        for piece in ("_check_", "_bind_", "_launch_"):
            assert callable(getattr(S.GraspStepper, piece + t.key)), piece + t.key
    assert (S.TABLETOP_TERMS, S.SCENE_TERMS, S.APPROACH_TERMS, S.PREGRASP_TERMS, S.SQUEEZE_TERMS, S.REACH_TERMS, S.ARM_TERMS, S.TRACK_TERMS,
            S.LIFT_TERMS) == (("E_prior", "E_wall"), ("E_scene",), ("E_approach",), ("E_pregrasp",), ("E_squeeze",), ("E_reach",), ("E_arm",),
                              ("E_track",), ("E_lift",))
    assert S.OBSTACLE_TERMS == ("E_scene", "E_approach", "E_pregrasp") and S.TERM_NAMES == FIXED


def test_merge_weights_key_order_and_refusals():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, merge_weights

    w = merge_weights(None)
    assert list(w) == MERGED_KEYS and list(merge_weights({"E_lift": 2.0, "E_dis": 50.0})) == MERGED_KEYS
    assert {k: w[k] for k in FIXED} == DEFAULT_WEIGHTS and all(w[k] == 0.0 for k in DECLARATION)
    for k in DECLARATION:
        assert merge_weights({k: 0.25})[k] == 0.25
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError, match=rf'weights\[{k!r}\] = .* must be >= 0'):
                merge_weights({k: bad})
    assert merge_weights({"E_dis": -1.0})["E_dis"] == -1.0  # the five fixed terms are not switched by their weight
    for k in ("E_manipulativity", "e_scene", "E_table", ""):
        with pytest.raises(ValueError, match="unknown energy term") as e:
            merge_weights({k: 1.0})
        assert f"(known: {', '.join(MERGED_KEYS)})" in str(e.value)  # the key order shows here


def test_select_tolerances_default_gates():
    from graspqp_amd.stepper import select_tolerances

    names = FIXED + DECLARATION
    inf = float("inf")
    assert select_tolerances(names) == [0.0 if k in GATED else inf for k in names]
    assert select_tolerances(names, {}) == [inf] * 15
    assert select_tolerances(FIXED + ("E_reach", "E_arm")) == [inf] * 6 + [0.0]  # only what is on
    with pytest.raises(ValueError, match="switched-off"):
        select_tolerances(FIXED, {"E_lift": 0.0})
    with pytest.raises(ValueError, match="NaN"):
        select_tolerances(names, {"E_lift": float("nan")})


def test_which_error_comes_first():
    """Every call is wrong twice; the message is the one of the term that stands earlier in the declaration order."""
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.stepper import GraspStepper

    hand = type("H", (), {"spec": get_hand_spec("allegro"), "L": 1, "J": 16, "S": 0})()
    objs = type("M", (), {"n_mesh": 1})()
    make = lambda weights, **kw: GraspStepper(hand, objs, torch.zeros(1, 8, 3), 4, 4, weights=weights, device="cpu", **kw)
    arm = dict(arm=ao.arm_spec("arm7"), arm_base=np.eye(4)[:3])
    cases = (
        ({"E_scene": 1.0}, dict(scene=None, scene_margin=-1.0), r'weights\["E_scene"\] > 0 needs scene=ops\.SceneSDF'),
        ({"E_pregrasp": 1.0, "E_squeeze": 1.0}, dict(squeeze_damping=0.0),
         r'weights\["E_pregrasp"\] > 0 needs pregrasp_scene= or scene=ops\.SceneSDF'),
        ({"E_squeeze": 1.0, "E_reach": 1.0}, dict(squeeze_damping=0.0), "squeeze_damping = 0.0 must be finite and > 0"),
        ({"E_reach": 1.0, "E_arm": 1.0}, {}, r'weights\["E_reach"\] > 0 needs arm=ops\.ArmSpec'),
        ({"E_arm": 1.0, "E_track": 1.0}, arm, r'weights\["E_arm"\] > 0 needs weights\["E_reach"\] > 0'),
        ({"E_track": 1.0, "E_lift": 1.0}, arm, r'weights\["E_track"\] > 0 needs weights\["E_reach"\] > 0'),
        ({"E_lift": 1.0}, dict(init_avoid_scene=True), r'weights\["E_lift"\] > 0 needs lift_scene= or scene=ops\.SceneSDF'),
    )
    for weights, kw, message in cases:
        with pytest.raises(ValueError, match=message):
            make(weights, **kw)
    # each half alone raises its own message: the calls above were wrong twice
    alone = (
        ({}, dict(scene_margin=-1.0), "scene_margin = -1.0 must be >= 0"),
        ({"E_squeeze": 1.0}, dict(squeeze_damping=0.0), "squeeze_damping"),
        ({"E_reach": 1.0}, {}, "needs arm="),
        ({"E_arm": 1.0, "E_reach": 1.0}, dict(arm=ro.arm_spec("arm7"), arm_base=np.eye(4)[:3]), "collision spheres"),
        ({"E_track": 1.0}, arm, r'weights\["E_track"\] > 0 needs weights\["E_reach"\] > 0'),
        ({}, dict(init_avoid_scene=True), "init_avoid_scene=True needs"),
        ({"E_approach": 1.0}, {}, r'weights\["E_approach"\] > 0 needs scene=ops\.SceneSDF'),
        ({"E_arm": 1.0, "E_reach": 1.0}, arm, r'weights\["E_arm"\] > 0 needs arm_scene= or scene=ops\.SceneSDF'),
        ({"E_reach": 1.0}, dict(arm_on_track=True, reach_stations=2, **arm), "arm_on_track=True needs"),
    )
    for weights, kw, message in alone:
        with pytest.raises(ValueError, match=message):
            make(weights, **kw)
