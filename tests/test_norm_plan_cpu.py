"""The launch plan of the BatchNorm family (NormPlan, csrc/lgs_norm.hip), held on the CPU through lgs_debug_norm_plan: no HIP
call, the one device query (co-resident workgroups of a grid-barrier kernel) is part of the question.

tests/golden/norm_plan_table.json was recorded from the code BEFORE the plan existed, through a shim that walked the `if` cascades
of bn_forward_t / bn_backward_t / bn_stats_t / bn_bwd_reduce_t (bn_fold_on -> fold_parts, fold_grid; bn_fused_on -> fused_cap's
clamp with the queried number injected -> fused_blocks and the inline fold of the conv partial rows; reduce_blocks /
stats_partials, the apply grid) and called lgs_bn_workspace_bytes, without launching.  Every row must still give the same path,
grids, rows per workgroup and fold counts, and may not need a larger workspace.

Independently of the table, the workspace layout of every row must be sound: 4-byte aligned, disjoint regions, each large enough
for what its kernel writes, inside lgs_bn_workspace_bytes(n, c) -- which the callers cache per (n, c) and which therefore may not
depend on the knobs, the dtype or the direction.

`python tests/test_norm_plan_cpu.py --record` rewrites the table from the library as built (only when a behaviour change is
intended).
"""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "norm_plan_table.json")

F32, BF16 = 0, 1
FWD, BWD, STATS, BWD_REDUCE = 0, 1, 2, 3
PATHS = {1: "fold", 2: "fused", 3: "three"}
BIG = 600000000                       # rows: past 2^31 elements at every channel count of the sweep
NS = [0, 1, 127, 128, 129, 5000, 16383, 19648, 65536, 81920, 327583, 1205389, BIG]
CS = [4, 8, 32, 96, 128, 200, 256, 512, 544, 2048]
PARTIAL_ROWS = [1, 77, 128, 4709]     # of the conv epilogue; 0 = statistics from x
CAPS = [0, 15, 16, 100, 1024]         # co-resident workgroups the device reports; 256 everywhere else
KNOBS = [("BN_FOLD", 0), ("BN_FOLD_MAX_MB", 0), ("BN_FOLD_MAX_MB", 1), ("BN_FOLD_MAX_MB", 24),
         ("BN_FOLD_PARTS", 0), ("BN_FOLD_PARTS", 1), ("BN_FOLD_PARTS", 64), ("BN_FOLD_PARTS", 65),
         ("BN_FOLD_GRID", 0), ("BN_FOLD_GRID", 1), ("BN_FOLD_GRID", 256),
         ("BN_FUSED", 0), ("BN_FUSED_MAX_MB", 0), ("BN_FUSED_MAX_MB", 6), ("BN_FUSED_MAX_MB", 64),
         ("BN_FUSED_FWD_MAX_MB", 6), ("BN_FUSED_FWD_MAX_MB", 24), ("BN_FUSED_BLOCKS", 1), ("BN_FUSED_BLOCKS", 64), ("BN_FUSED_BLOCKS", 512)]

QUERY_COLS = ["knob", "knob_value", "direction", "n", "c", "dtype", "conv_partial_rows", "resident_cap"]
EQUAL_COLS = ["path", "from_partials", "reduce_grid", "rows_per_block", "partial_rpb", "fold_rows", "fold_grid", "apply_grid"]
COLS = QUERY_COLS + EQUAL_COLS + ["workspace_bytes"]
REGIONS = ("partials", "sums", "spill")


def supported(c, dtype):
    """the channel counts the kernels take: whole 16-byte vectors, at most 256 of them per row"""
    w = 8 if dtype == BF16 else 4
    return c % w == 0 and c // w <= 256


def sweep():
    """the pruned cross product, in a fixed order: -> [(knob, value, direction, n, c, dtype, conv_partial_rows, resident_cap)]"""
    rows = []
    shapes = [(c, dt) for c in CS for dt in (BF16, F32) if supported(c, dt)]
    for d in (FWD, BWD):                                            # every size x every shape, statistics from x
        rows += [("", 0, d, n, c, dt, 0, 256) for n in NS for c, dt in shapes]
    for d in (STATS, BWD_REDUCE):                                   # the halves never leave the three-launch path
        rows += [("", 0, d, n, c, dt, 0, 256) for n in NS for c, dt in ((32, BF16), (96, BF16), (96, F32), (512, BF16))]
    for d in (FWD, STATS):                                          # statistics from the conv epilogue's rows
        rows += [("", 0, d, n, c, dt, pr, 256) for pr in PARTIAL_ROWS for n in (0, 5000, 81920, 327583, 1205389)
                 for c, dt in ((96, BF16), (96, F32), (256, BF16))]
    for d in (FWD, BWD):                                            # what the device reports
        rows += [("", 0, d, n, 96, dt, 0, cap) for cap in CAPS for n in (1, 5000, 81920, 327583, 1205389) for dt in (BF16, F32)]
    for knob, value in KNOBS:
        for d in (FWD, BWD):
            rows += [(knob, value, d, n, 96, dt, 0, 256) for n in (5000, 19648, 81920, 327583) for dt in (BF16, F32)]
        if knob in ("BN_FUSED_FWD_MAX_MB", "BN_FUSED_BLOCKS"):      # the one-launch forward on the conv epilogue's rows
            rows += [(knob, value, FWD, n, 96, BF16, pr, 256) for n in (5000, 81920) for pr in (77, 4709)]
    return rows


def query(row):
    """one sweep row, under its knob -> (the dict of COLS as the library answers now, the plan)"""
    from languagegroundedsemseg_amd import engine
    knob, value, d, n, c, dt, pr, cap = row
    q = engine.NormPlanQuery(d, c, dt, pr, cap, n)
    info = engine.NormPlanInfo()
    with engine.tuning(**({knob: value} if knob else {})):
        engine.check(engine.lib().lgs_debug_norm_plan(ctypes.byref(q), ctypes.byref(info)))
    out = dict(zip(QUERY_COLS, row))
    for col in EQUAL_COLS + ["workspace_bytes"]:
        out[col] = getattr(info, col)
    return out, info


@pytest.fixture(scope="module")
def answers():
    from languagegroundedsemseg_amd import build
    build.build()
    return [query(row) for row in sweep()]


@pytest.fixture(scope="module")
def table():
    t = json.load(open(TABLE))
    assert t["columns"] == COLS
    return [dict(zip(COLS, r)) for r in t["rows"]]


def test_table_is_the_sweep(table):
    want = sweep()
    assert len(table) == len(want) and 300 <= len(want) <= 3000
    assert os.path.getsize(TABLE) < (1 << 20)
    for rec, row in zip(table, want):
        assert tuple(rec[c] for c in QUERY_COLS) == tuple(row)


def test_table_covers_every_path(table):
    """every path of every direction, statistics from x and from the conv epilogue, both sides of every bound and cap"""
    def rows(path, **kw):
        return [r for r in table if PATHS[r["path"]] == path and all(r[k] == v for k, v in kw.items())]
    for d in (FWD, BWD):
        for dt in (BF16, F32):
            assert rows("fold", direction=d, dtype=dt) and rows("fused", direction=d, dtype=dt) and rows("three", direction=d, dtype=dt), (d, dt)
    assert rows("fused", direction=FWD, from_partials=1) and rows("three", direction=FWD, from_partials=1) and rows("three", direction=STATS, from_partials=1)
    assert not rows("fold", from_partials=1) and not rows("fold", n=0)
    assert {PATHS[r["path"]] for r in table if r["direction"] in (STATS, BWD_REDUCE)} == {"three"}
    assert rows("three", n=0, apply_grid=0) and rows("three", apply_grid=4096) and rows("three", reduce_grid=512)
    assert rows("fused", reduce_grid=256, resident_cap=1024) and rows("fused", reduce_grid=100) and rows("fused", reduce_grid=16)
    assert not rows("fused", resident_cap=15) and not rows("fused", resident_cap=0)
    assert {(r["fold_rows"], r["partial_rpb"]) for r in table if r["from_partials"]} == {(1, 1), (77, 1), (128, 1), (128, 37)}   # 4709 rows: 37 at a time
    assert any(r["n"] * r["c"] >= 1 << 31 for r in table)
    # the knobs at work: each value changes the decision of at least one row against the same query without it -- except the
    # defaults and the values the plan reads as the default (parts outside 1 .. 64, grid 0, more blocks than the device holds)
    inert = {("BN_FOLD_PARTS", 0), ("BN_FOLD_PARTS", 64), ("BN_FOLD_PARTS", 65), ("BN_FOLD_GRID", 0), ("BN_FOLD_GRID", 256), ("BN_FUSED_BLOCKS", 512)}
    base = {tuple(r[c] for c in QUERY_COLS[2:]): r for r in table if not r["knob"]}
    for knob, value in KNOBS:
        mine = [r for r in table if (r["knob"], r["knob_value"]) == (knob, value)]
        changed = [r for r in mine if any(r[c] != base[tuple(r[k] for k in QUERY_COLS[2:])][c] for c in EQUAL_COLS)]
        assert mine and bool(changed) == ((knob, value) not in inert), (knob, value)


def test_plan_equals_the_recorded_decisions(answers, table):
    assert len(answers) == len(table)
    for (got, _), rec in zip(answers, table):
        for c in EQUAL_COLS:
            assert got[c] == rec[c], "%s: %s = %s, recorded %s" % ({k: rec[k] for k in QUERY_COLS}, c, got[c], rec[c])


def test_workspace_does_not_grow(answers, table):
    for (got, _), rec in zip(answers, table):
        assert 0 < got["workspace_bytes"] <= rec["workspace_bytes"], ({k: rec[k] for k in QUERY_COLS}, got["workspace_bytes"], rec["workspace_bytes"])


def test_workspace_layout_is_sound(answers):
    """independent of the table: regions that hold what the kernels write, disjoint, inside the one size the callers keep per (n, c)"""
    from languagegroundedsemseg_amd import engine
    for got, info in answers:
        where = {k: got[k] for k in QUERY_COLS}
        d, n, c, path = got["direction"], got["n"], got["c"], PATHS[info.path]
        row = 2 * c * 4                                        # one partial row: [2][c] floats (k_colreduce, k_partial_reduce, colreduce_slab)
        ws = engine.lib().lgs_bn_workspace_bytes(n, c)         # asked under the DEFAULT knobs, as a caller that cached it did
        assert info.workspace_bytes == ws, (where, info.workspace_bytes, ws)
        used = sorted(((r, getattr(info, r).offset, getattr(info, r).bytes) for r in REGIONS if getattr(info, r).bytes > 0), key=lambda r: r[1])
        for r, o, b in used:
            assert o % 4 == 0 and o >= 0 and o + b <= info.bytes_total <= ws, (where, r, o, b, info.bytes_total, ws)
        for (r0, o0, b0), (r1, o1, b1) in zip(used, used[1:]):
            assert o0 + b0 <= o1, (where, r0, r1)
        # the launches cover their rows, within the caps of the kernels that own them
        if info.reduce_grid:
            assert info.reduce_grid * info.rows_per_block >= n and (info.reduce_grid - 1) * info.rows_per_block < max(n, 1), where
            assert info.reduce_grid <= {"fold": 64, "fused": min(256, max(got["resident_cap"], 0)), "three": 512}[path], where
            assert path != "fused" or got["resident_cap"] >= 16, where
        else:
            assert path == "three" and info.from_partials, where
        if info.from_partials:
            pr = got["conv_partial_rows"]
            assert d in (FWD, STATS) and pr > 0 and info.fold_rows <= 128, where
            assert info.fold_rows * info.partial_rpb >= pr > (info.fold_rows - 1) * info.partial_rpb, where
        else:
            assert info.partial_rpb == 0 and info.fold_rows == info.reduce_grid, where
        # what the kernels write: fold_rows partial rows; k_fold_bwd / k_bn_bwd_fused sums[0 .. 2c); lgs_bn_backward_reduce's
        # unwanted dbeta at spill[0 .. c), dgamma at spill[c .. 2c)
        assert info.partials.bytes >= info.fold_rows * row > 0, where
        assert info.sums.bytes >= (row if d == BWD and path != "fold" else 0) and bool(info.sums.bytes) == (d == BWD and path != "fold"), where
        assert info.spill.bytes >= (row if d == BWD_REDUCE else 0) and bool(info.spill.bytes) == (d == BWD_REDUCE), where
        assert (info.fold_grid == (c + 15) // 16) if path == "three" else info.fold_grid == 0, where      # 16 channels per k_fold_* workgroup
        w = 8 if got["dtype"] == BF16 else 4
        if path == "fold":
            assert 1 <= info.apply_grid <= 256 or got["knob"] == "BN_FOLD_GRID", where
        elif path == "three" and d in (FWD, BWD):
            assert info.apply_grid == min(-(-n * (c // w) // 256), 4096), where
        else:
            assert info.apply_grid == 0, where


def test_unsupported_channel_counts_are_refused():
    from languagegroundedsemseg_amd import build, engine
    build.build()
    for c, dt in ((4, BF16), (2048, F32), (100, BF16), (6, F32)):
        q, info = engine.NormPlanQuery(FWD, c, dt, 0, 256, 5000), engine.NormPlanInfo()
        assert engine.lib().lgs_debug_norm_plan(ctypes.byref(q), ctypes.byref(info)) != 0, (c, dt)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        sys.path.insert(0, ROOT)
        rows = [[got[c] for c in COLS] for got, _ in map(query, sweep())]
        with open(TABLE, "w") as f:
            f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(COLS), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
        print("recorded", len(rows), "rows")
