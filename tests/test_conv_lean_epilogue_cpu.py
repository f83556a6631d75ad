"""CONV_LEAN_EPI picks an INSTANCE of k_conv_gather (with or without the BatchNorm statistics epilogue), never a plan: the knob is in
the tuning table with default 1, and lgs_debug_conv_plan answers byte for byte the same with it at 0 and at 1 for the shapes the
128-column tile (id 7) serves -- tile, packed image, grid, split, statistic rows, workspace regions and the public queries."""
import ctypes

import pytest

from test_conv_plan_cpu import BF16, ask, make_views

# (kind, n_pad, cin, cout, op, SMALL_CFG): the tile-7 shapes of tests/test_gpu_conv_lean_epilogue.py and of the 8-scene step
CASES = [
    ("k3", 1200128, 128, 96, 1, 0), ("k1", 1200128, 128, 96, 1, 0), ("k3", 65792, 128, 96, 1, 0),      # the 96 -> 128 dgrad (nc = 3)
    ("k3", 82176, 128, 128, 0, 0), ("k3", 82176, 128, 128, 1, 0),                                      # 128 -> 128 at level 2
    ("k3", 19712, 256, 256, 0, 0), ("k3", 19712, 256, 256, 1, 0),                                      # 256 -> 256 at level 3
    ("k3", 1200128, 96, 96, 0, 0),                                                                     # the tile-2 control
    ("k3", 2816, 128, 96, 1, 7), ("k1", 2816, 128, 96, 1, 7), ("k3", 2816, 128, 128, 0, 7), ("k3", 2816, 256, 256, 1, 7),
    ("k3", 2816, 96, 100, 0, 7),
]


@pytest.fixture(scope="module")
def engine():
    from languagegroundedsemseg_amd import build, engine
    build.build()
    return engine


def test_the_knob_is_in_the_tuning_table(engine):
    rows = {name: (default, doc) for name, default, _, doc in engine.tuning_table()}
    assert rows["CONV_LEAN_EPI"][0] == 1 and "statistics" in rows["CONV_LEAN_EPI"][1]


@pytest.mark.parametrize("kind,n_pad,cin,cout,op,small", CASES)
def test_the_plan_does_not_depend_on_the_knob(engine, kind, n_pad, cin, cout, op, small):
    views = make_views(kind, n_pad)
    plans = {}
    for lean in (0, 1, 2):
        for epi in (0, 1 if op == 0 else 2):
            with engine.tuning(CONV_LEAN_EPI=lean, SMALL_CFG=small):
                plans[lean, epi] = bytes(ask(views, op, 0, cin, cout, BF16, epi))
    for epi in (0, 1 if op == 0 else 2):
        assert plans[0, epi] == plans[1, epi] == plans[2, epi]
    info = engine.ConvPlanInfo.from_buffer_copy(plans[1, 0])
    assert info.path == 4
    if (cin, cout) != (96, 96):
        assert info.tile_id == 7, info.tile_id
