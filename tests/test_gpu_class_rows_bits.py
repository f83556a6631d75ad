"""The class-row kernels (k_ce_fwd_bwd, k_focal_fwd_bwd, k_seg_metrics; csrc/lgs_classrows.h) give, bit for bit, what they gave
before their accesses and host dispatch were unified: SHA-256 digests of every output, recorded on an MI355X from the commit before the change
(tests/golden/class_rows_bits.json, written by tests/golden/make_class_rows_bits.py), against the same runs of the tree under test.
The generator is imported for the inputs and the runs, so both sides execute the same lines.  Math-library code (expf, log1pf) may
change between toolchains: under another HIP version than the recorded one the comparison says nothing and the tests skip."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.parity("digests recorded from the parent commit's build")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_class_rows_bits", os.path.join(GOLDEN, "make_class_rows_bits.py"))
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


def test_fixture_covers_every_case(recorded):
    want = {gen.case_name(dtype, c, n) for dtype, c in gen.SHAPES for n in gen.row_counts(c, dtype)}
    assert set(recorded) == want


@pytest.mark.parametrize("dtype,c", gen.SHAPES, ids=[gen.case_name(d, c, 0).rsplit("-", 1)[0] for d, c in gen.SHAPES])
def test_outputs_are_bit_identical_to_the_recorded_ones(recorded, dtype, c):
    bad = []
    for n in gen.row_counts(c, dtype):
        name = gen.case_name(dtype, c, n)
        got, want = gen.run_case(dtype, c, n), recorded[name]
        assert set(got) == set(want), name
        bad += ["%s/%s" % (name, k) for k in sorted(want) if got[k] != want[k]]
    assert not bad, "outputs differ from the recorded bits: " + ", ".join(bad)
