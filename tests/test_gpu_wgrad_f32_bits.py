"""The fp32 weight-gradient kernels (k_wgrad_f32, k_wgrad_f32_lds, k_wgrad_f32s_lds; csrc/lgs_wgrad.hip) give, bit for bit, what they
gave before they were rewritten over one pair-list skeleton: SHA-256 digests of every gradient, recorded on an MI355X from the commit
before the change (tests/golden/wgrad_f32_bits.json, written by tests/golden/make_wgrad_f32_bits.py), against the same runs of the
tree under test.  The generator is imported for the inputs and the runs, so both sides execute the same lines; its runs also assert
through engine.dispatch_counts() that every case reaches the kernel and the column-tile width it is meant for.  The kernels hold
no math-library code, but the compiler's contraction choices may change between toolchains: under another HIP version than the
recorded one the comparison says nothing and the tests skip."""
import importlib.util
import json
import os

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.parity("digests recorded from the parent commit's build")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_wgrad_f32_bits", os.path.join(GOLDEN, "make_wgrad_f32_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(gen.PATH) as f:
        doc = json.load(f)
    env = gen.environment()
    assert doc["arch"] == env["arch"], "digests recorded on %s, running on %s" % (doc["arch"], env["arch"])
    if doc["hip"] != env["hip"]:
        pytest.skip("digests recorded under HIP %s, running HIP %s" % (doc["hip"], env["hip"]))
    return doc["cases"]


@pytest.fixture(scope="module")
def maps():
    return gen.Maps()


def _same_bits(name, got, want):
    assert set(got) == set(want) == {"knob%d" % m for m in gen.KNOBS}, name
    bad = ["%s/%s" % (name, k) for k in sorted(want) if got[k] != want[k]]
    assert not bad, "gradients differ from the recorded bits: " + ", ".join(bad)


def test_fixture_covers_every_case(recorded):
    assert set(recorded) == set(gen.all_case_names())


def test_the_scenes_have_the_sizes_the_cases_are_meant_for(maps):
    assert maps.n_voxels("big") > 4096 and 512 < maps.n_voxels("small") < 768


@pytest.mark.parametrize("scene", list(gen.SCENES))
@pytest.mark.parametrize("case", gen.MAP_CASES, ids=[gen.case_name("", *c[:3], c[4])[1:] for c in gen.MAP_CASES])
def test_map_gradients_are_bit_identical_to_the_recorded_ones(recorded, maps, scene, case):
    name = gen.case_name(scene, *case[:3], case[4])
    _same_bits(name, gen.run_map_case(maps, scene, *case), recorded[name])


def test_clip_anchor_gradient_is_bit_identical_to_the_recorded_one(recorded):
    _same_bits("clip-anchors", gen.run_clip_case(), recorded["clip-anchors"])
