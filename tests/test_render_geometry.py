"""The drawn robot is the simulated robot: the committed ss_visual_tables.hpp is what tools/gen_model_tables.py produces from
model.visual_geoms now, and the primitives' masses add up to model.build()'s body masses (docs/RENDER.md 2)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_committed_visual_tables_equal_the_generator_output():
    import gen_model_tables as gen
    assert open(os.path.join(ROOT, "steppingstone_amd", "csrc", "ss_visual_tables.hpp")).read() == gen.gen_visual_hpp()


def _mass(t, prm, density):
    if t == "sphere":
        return density * 4.0 / 3.0 * np.pi * float(prm["r"]) ** 3
    if t == "box":
        return density * 8.0 * np.prod(prm["half"])
    r, L = float(prm["r"]), np.linalg.norm(prm["p1"] - prm["p0"])
    return density * (np.pi * r * r * L + 4.0 / 3.0 * np.pi * r ** 3)


def test_primitive_masses_are_the_simulated_body_masses():
    from steppingstone_amd import model
    for kind in ("walker3d", "mike"):
        P = model.params(kind, model.identified(kind))
        m = model.build(kind)
        groups = model.body_groups(kind)
        geoms = model.visual_geoms(kind)
        assert len(geoms) == 17 and all(t in ("capsule", "sphere", "box") for _, t, _ in geoms)
        for b in range(model.NB):
            mine = [(t, prm) for body, t, prm in geoms if body == b]
            if m["mass"][b] == 0:
                assert not mine and groups[b] is None, (kind, b)
                continue
            drawn = sum(_mass(t, prm, P["density"]) for t, prm in mine) * P["mass_scale"] * P["mass_mult"][groups[b]]
            assert abs(drawn - m["mass"][b]) <= 1e-9 * m["mass"][b], (kind, b, drawn, m["mass"][b])


def test_visual_geoms_follow_overrides():
    from steppingstone_amd import model
    g0 = {(b, t): prm for b, t, prm in model.visual_geoms("walker3d")}
    g1 = {(b, t): prm for b, t, prm in model.visual_geoms("walker3d", overrides={"thigh": 0.40})}
    assert np.isclose(g1[(6, "capsule")]["p1"][2], -0.40) and not np.isclose(g0[(6, "capsule")]["p1"][2], -0.40)
