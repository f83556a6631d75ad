"""Which instance of k_conv_gather a planned launch runs (gather_instance + the instance table, csrc/lgs_conv.hip), held on the CPU
through lgs_debug_conv_gather_instance: no HIP call, the kernel maps are synthetic.

tests/golden/conv_instance_table.json was recorded from the code BEFORE the table and the choice function existed (the `lean`,
`scl` and `row1` expressions, the 12-row walk switch and the ONEBUF flag spelled inside launch_gather), through a throw-away query
that evaluated those expressions as they stood.  Inputs: every row of test_conv_plan_cpu.sweep() that plans k_conv_gather (plus EXTRA), without
statistics and -- forward launches whose plan has statistic rows -- with them, under CONV_LEAN_EPI 0 / 1 / 2 x CONV_SLAB_TRIM
0 / 1 / 2 x CONV_ROW_TRIM 0 / 1.  Every launch must still get the same tile, walk, one-piece row, epilogue variant and slab buffers.

Independently of the table: the launch-site names the engine registers are the ones tests/helpers.py spells (the GPU tests and the
profiles key on them), and the shapes of tests/test_gpu_conv_zero_loads.py and tests/test_conv_lean_epilogue_cpu.py get the
instances those tests expect, with the expectations copied from there.

`python tests/test_conv_instance_cpu.py --record` rewrites the table from the library as built (only when a change of the
instance choice is intended).
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

from helpers import GATHER_LEAN_COUNTER, GATHER_TILES
from test_conv_lean_epilogue_cpu import CASES as LEAN_CASES
from test_conv_plan_cpu import BF16, F32, ask, make_views, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_instance_table.json")
KNOBS = list(itertools.product((0, 1, 2), (0, 1, 2), (0, 1)))        # CONV_LEAN_EPI, CONV_SLAB_TRIM, CONV_ROW_TRIM
FIELDS = ["tile_id", "scl", "row1", "bn", "onebuf"]
# (tile, chunks per slab, one-piece row) of every slab walk of the instance table
WALKS = {(0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 3, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (7, 1, 0), (7, 3, 0)}
# the walks no model shape of the sweep reaches: 96 -> 64 forward (tile 1, three chunks on 4-chunk slabs) and its dgrad (tile 2, two)
EXTRA = [("", 0, "k3", 1200128, 96, 64, BF16, 0, 0, 0), ("", 0, "k3", 1200128, 96, 64, BF16, 1, 0, 0)]
DT = {BF16: "[T=unsignedshort]", F32: "[T=float]", "f32s": "[T=lgs::f32s_t]"}


def instance(views, op, tr, cin, cout, dtype, epi, stats):
    """-> ConvGatherInstance of the launch of this query"""
    from languagegroundedsemseg_amd import engine
    ks, fwd, bwd = views
    q = engine.ConvPlanQuery(fwd, bwd, ks, op, tr, cin, cout, dtype, epi)
    out = engine.ConvGatherInstance()
    engine.check(engine.lib().lgs_debug_conv_gather_instance(ctypes.byref(q), stats, ctypes.byref(out)))
    return out


def inputs():
    """-> [(sweep row, with statistics)]: the sweep rows (and EXTRA) that plan k_conv_gather, in sweep order"""
    from languagegroundedsemseg_amd import engine
    out = []
    for row in sweep() + EXTRA:
        knob, value, kind, n_pad, cin, cout, dtype, op, tr, epi = row
        with engine.tuning(**({knob: value} if knob else {})):
            info = ask(make_views(kind, n_pad), op, tr, cin, cout, dtype, epi)
        if info.path == 4:
            out += [(row, 0)] + ([(row, 1)] if op == 0 and info.bn_rows > 0 and info.q_bn_partial_rows > 0 else [])
    return out


def answer(row, stats, fn=instance):
    """the instance under each of KNOBS -> [[tile_id, scl, row1, bn, onebuf]]"""
    from languagegroundedsemseg_amd import engine
    knob, value, kind, n_pad, cin, cout, dtype, op, tr, epi = row
    views = make_views(kind, n_pad)
    got = []
    for lean, slab, rowtrim in KNOBS:
        knobs = dict(CONV_LEAN_EPI=lean, CONV_SLAB_TRIM=slab, CONV_ROW_TRIM=rowtrim)
        if knob:
            knobs[knob] = value
        with engine.tuning(**knobs):
            g = fn(views, op, tr, cin, cout, dtype, epi, stats)
        got.append([int(getattr(g, f)) for f in FIELDS])
    return got


def record(fn=instance):
    """the table as the library answers now: distinct instances once, a row per input with one index per knob setting"""
    distinct, rows = [], []
    for row, stats in inputs():
        idx = []
        for g in answer(row, stats, fn):
            if g not in distinct:
                distinct.append(g)
            idx.append(distinct.index(g))
        rows.append(list(row) + [stats, idx])
    with open(TABLE, "w") as f:
        f.write('{"fields": %s,\n "knobs": %s,\n "instances": %s,\n "rows": [\n%s\n]}\n' % (
            json.dumps(FIELDS), json.dumps(KNOBS), json.dumps(distinct), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
    return len(rows)


@pytest.fixture(scope="module")
def engine():
    from languagegroundedsemseg_amd import build, engine
    build.build()
    return engine


@pytest.fixture(scope="module")
def table(engine):
    t = json.load(open(TABLE))
    assert t["fields"] == FIELDS and [tuple(k) for k in t["knobs"]] == KNOBS
    return t


def test_table_is_the_sweep(engine, table):
    want = inputs()
    assert len(table["rows"]) == len(want) and len(want) >= 300
    for rec, (row, stats) in zip(table["rows"], want):
        assert tuple(rec[:10]) == tuple(row) and rec[10] == stats and len(rec[11]) == len(KNOBS)


def test_table_covers_every_tile_and_every_walk(table):
    inst = [dict(zip(FIELDS, g)) for g in table["instances"]]
    used = {i for rec in table["rows"] for i in rec[11]}
    assert used == set(range(len(inst)))
    assert {g["tile_id"] for g in inst} == set(GATHER_TILES)
    assert {(g["tile_id"], g["scl"], g["row1"]) for g in inst if g["scl"]} == WALKS
    lean = {(g["tile_id"], g["scl"], g["row1"]) for g in inst if not g["bn"]}
    assert lean == {(t, 0, 0) for t in (0, 1, 2, 6, 7, 16)} | WALKS                  # every instance that has a lean twin ran as one
    assert {(g["tile_id"], g["scl"]) for g in inst if g["onebuf"]} == {(7, 3)} and all(not g["bn"] for g in inst if g["onebuf"])
    with_stats = {i for rec in table["rows"] if rec[10] for i in rec[11]}
    assert with_stats and all(inst[i]["bn"] for i in with_stats)


def test_instance_equals_the_recorded_choice(engine, table):
    for rec in table["rows"]:
        got = answer(tuple(rec[:10]), rec[10])
        want = [table["instances"][i] for i in rec[11]]
        for knobs, g, w in zip(KNOBS, got, want):
            assert g == w, "%s statistics %d, (lean, slab trim, row trim) = %s: %s, recorded %s" % (rec[:10], rec[10], knobs, g, w)


def own(tile, dt=BF16):
    return "k_conv_gather<T,%s> %s" % (GATHER_TILES[tile], DT[dt])


def walk(scl, tile, row1=False):
    return "SlabWalk<%d,%s>::%s" % (scl, "true" if row1 else "false", own(tile))


def test_launch_site_names(engine, table):
    """every tile id (bf16, and fp32 / split-fp32 where the tile has that instance) and every walk: the registered name is the one
    the GPU tests spell, whichever epilogue variant runs; the numbers of the row are the numbers in the name"""
    seen = set()
    for rec in table["rows"]:
        knob, value, kind, n_pad, cin, cout, dtype, op, tr, epi = rec[:10]
        for fp32_split in ((1, 0) if dtype == F32 else (1,)):
            for lean, slab in ((1, 1), (0, 2), (1, 0)):
                knobs = dict(CONV_LEAN_EPI=lean, CONV_SLAB_TRIM=slab, FP32_SPLIT=fp32_split)
                if knob:
                    knobs[knob] = value
                with engine.tuning(**knobs):
                    g = instance(make_views(kind, n_pad), op, tr, cin, cout, dtype, epi, rec[10])
                    dt = dtype if dtype == BF16 or not engine.tuning_get("FP32_SPLIT") else "f32s"
                want = walk(g.scl, g.tile_id, bool(g.row1)) if g.scl else own(g.tile_id, dt)
                assert g.site.decode() == want, (rec[:10], g.site, want)
                # "(kF32?a:b)" of the site text, evaluated for the dtype (a and b are never 0)
                nums = [eval(x.replace("?", " and ").replace(":", " or "), {"kF32": dtype == F32}) for x in GATHER_TILES[g.tile_id].split(",")]
                assert [g.rb, g.ncb, g.wm, g.wn, g.sc, g.d] == nums, (rec[:10], nums)
                seen.add((g.tile_id, g.scl, g.row1, dt))
    assert {t for t, _, _, dt in seen if dt == BF16} == set(GATHER_TILES) and {(t, s, r) for t, s, r, _ in seen if s} == WALKS
    assert {t for t, _, _, dt in seen if dt == F32} == {t for t, _, _, dt in seen if dt == "f32s"} >= {0, 1, 2, 3, 4, 5}
    assert GATHER_LEAN_COUNTER == "k_conv_gather:no_statistics_epilogue"


# tests/test_gpu_conv_zero_loads.py, SHAPES: one 3^3 map of 70 000 voxels (70 144 padded rows), bf16.  (cin, cout) -> the forward
# site under CONV_SLAB_TRIM=1 CONV_ROW_TRIM=1 (None: no walk, the tile's own instance), the forward site with both at 0, and the
# same two for the dgrad (a cout -> cin reduction)
T0, T1, T2, T7 = 0, 1, 2, 7
ZERO_LOAD_SHAPES = {
    (96, 96): (walk(3, T2), own(T2), walk(3, T2), own(T2)),
    (128, 96): (None, own(T2), walk(3, T7), own(T7)),
    (32, 32): (walk(1, T0), own(T0), walk(1, T0), own(T0)),
    (64, 64): (walk(2, T1), own(T1), walk(2, T1), own(T1)),
    (3, 32): (walk(1, T0, True), own(T0), walk(1, T0), own(T0)),
    (192, 128): (None, own(T7), None, own(T2)),
    (192, 96): (walk(3, T2), own(T2), walk(3, T2), own(T2)),
    (160, 96): (None, own(T2), walk(3, T7), own(T7)),
}


@pytest.mark.parametrize("cin,cout", list(ZERO_LOAD_SHAPES))
def test_the_shapes_of_the_zero_load_test(engine, cin, cout):
    fon, foff, don, doff = ZERO_LOAD_SHAPES[(cin, cout)]
    views = make_views("k3", 70144)
    for op, on, off in ((0, fon, foff), (1, don, doff)):
        with engine.tuning(CONV_SLAB_TRIM=1, CONV_ROW_TRIM=1):
            assert instance(views, op, 0, cin, cout, BF16, 0, 0).site.decode() == (on or off)
        with engine.tuning(CONV_SLAB_TRIM=0, CONV_ROW_TRIM=0):
            assert instance(views, op, 0, cin, cout, BF16, 0, 0).site.decode() == off
    if (cin, cout) == (128, 96):      # test_tile7_three_single_chunk_slabs
        with engine.tuning(CONV_SLAB_TRIM=2, CONV_ROW_TRIM=1):
            assert instance(views, 1, 0, cin, cout, BF16, 0, 0).site.decode() == walk(1, T7)
    if (cin, cout) == (3, 32):        # test_row_trim_alone
        with engine.tuning(CONV_SLAB_TRIM=1, CONV_ROW_TRIM=0):
            assert instance(views, 0, 0, cin, cout, BF16, 0, 0).site.decode() == walk(1, T0)


# tests/test_conv_lean_epilogue_cpu.py, CASES, in its order: does the launch run the instance WITHOUT the statistics epilogue under
# CONV_LEAN_EPI=1?  Tile 7 does on grids above 512 workgroups (9 376, 9 376, 514, 642, 642), not on level 3 of the 8-scene batch
# (308) nor on the 22-row-tile map of tests/test_gpu_conv_lean_epilogue.py; tile 2 always.  Knob 2: every one; knob 0: none
LEAN_UNDER_KNOB_1 = [True, True, True, True, True, False, False, True, False, False, False, False, False]


@pytest.mark.parametrize("case,lean1", list(zip(LEAN_CASES, LEAN_UNDER_KNOB_1)))
def test_the_cases_of_the_lean_epilogue_test(engine, case, lean1):
    kind, n_pad, cin, cout, op, small = case
    views = make_views(kind, n_pad)
    tile = 2 if (cin, cout) == (96, 96) else 7
    for knob, lean in ((0, False), (1, lean1), (2, True)):
        with engine.tuning(CONV_LEAN_EPI=knob, SMALL_CFG=small):
            g = instance(views, op, 0, cin, cout, BF16, 0, 0)
            assert (g.tile_id, bool(g.bn)) == (tile, not lean), (case, knob, g.tile_id, g.bn)
            nc = ((cin if op == 0 else cout) + 31) // 32
            assert (g.scl, bool(g.onebuf)) == ((3, lean) if tile == 7 and nc == 3 else (3, False) if tile == 2 else (0, False))
            if op == 0 and ask(views, op, 0, cin, cout, BF16, 1).bn_rows > 0:       # with statistics: the same tile and walk, never lean
                s = instance(views, op, 0, cin, cout, BF16, 1, 1)
                assert (s.tile_id, s.scl, s.bn, s.onebuf, s.site) == (tile, g.scl, 1, 0, g.site)
    if (kind, n_pad, cin, cout) == ("k3", 19712, 256, 256):
        assert ask(views, op, 0, cin, cout, BF16, 0).grid_x * ask(views, op, 0, cin, cout, BF16, 0).grid_y == 308


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        sys.path.insert(0, ROOT)
        print("recorded", record(), "rows")
