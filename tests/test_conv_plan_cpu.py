"""The launch plan of the forward / dgrad convolutions (ConvPlan, csrc/lgs_conv.hip), held on the CPU through
lgs_debug_conv_plan: no HIP call, the kernel maps are synthetic.

tests/golden/conv_plan_table.json was recorded from the code BEFORE the plan existed (tile choice, slot split, statistic
rows and workspace offsets derived separately in conv_gather_op, launch_gather, bn_partial_rows_t, pack_desc_t,
packed_region_bytes and lgs_conv_workspace_bytes), through a shim over those functions.  Every row must still give the same
path, tile, packed-image layout, grid, split and public answers, and may not need a larger workspace.

Independently of the table, the workspace layout of every row must be sound (aligned, disjoint regions inside the size the
public query reports, the packed image inside its region): the guard the out-of-bounds packed image of SMALL_CFG 12 / 13
never had.

`python tests/test_conv_plan_cpu.py --record` rewrites the table from the library as built (only when a behaviour change is
intended).
"""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")

N_PADS = [0, 256, 4096, 16384, 19712, 65536, 1200128]          # multiples of 256: empty .. the 1.2 M-point batch
# conv shapes (cin, cout) of Res16UNet34C / 34D / InsSegRes16UNet34C / 14A (languagegroundedsemseg_amd/models.py), by kernel size
SHAPES_K3 = [(64, 64), (256, 256), (3, 32), (32, 32), (32, 64), (64, 128), (128, 128), (128, 256), (384, 256), (192, 128), (128, 96),
             (96, 96), (384, 128), (160, 96), (320, 256), (288, 256), (544, 512), (512, 512)]
SHAPES_K1 = [(96, 200), (128, 96), (32, 64), (64, 128), (128, 256), (384, 256), (192, 128), (96, 96), (96, 3), (160, 96), (320, 256),
             (288, 256), (544, 512), (512, 512), (512, 200)]       # block downsamples, the class / CLIP heads, the offset heads
SHAPES_K2 = [(32, 32), (256, 256), (64, 64), (128, 128), (256, 128), (128, 96), (96, 96), (256, 512)]    # stride-2 convs and transposed convs
SHAPES_ODD = [(3, 32), (32, 3), (5, 64), (64, 5), (13, 13), (200, 96), (96, 200), (200, 200)]
KNOBS = [("SMALL_CFG", v) for v in (3, 5, 7, 9, 10, 11, 12, 13)] + \
        [("CONV_SPLIT", 0), ("CONV_WIDE", 0), ("HEAD_TILE", 1), ("FP32_SPLIT", 0), ("POINTWISE", 0), ("POINTWISE", 2)]
PATHS = {0: "empty", 1: "pointwise", 2: "pointwise_f32", 3: "wide", 4: "gather"}
F32, BF16 = 0, 1

QUERY_COLS = ["knob", "knob_value", "kind", "n_pad", "cin", "cout", "dtype", "op", "transposed", "epilogue"]
EQUAL_COLS = ["path", "tile_id", "ncp", "nbp", "gc", "grid_x", "grid_y", "grid_z", "split", "bn_rows", "can_accumulate",
              "q_bn_partial_rows", "q_can_accumulate",
              "pd_bytes", "pd_total", "pd_K", "pd_cin_w", "pd_cout_w", "pd_transposed", "pd_mirror", "pd_g_real", "pd_o_real", "pd_ncp",
              "pd_nbp", "pd_dtype"]
INFO_COLS = ["pad_input", "scratch_out"]
COLS = QUERY_COLS + EQUAL_COLS + INFO_COLS + ["workspace_bytes"]


def make_views(kind, n_pad):
    """(ks, fwd, bwd) as lgs_manager_kernel_map builds them; n_pad is the padded size of the map the view walks"""
    from languagegroundedsemseg_amd.engine import ConvPlanView as V
    n = max(n_pad - 100, 0)                       # rows of the map: not a multiple of anything
    if kind == "k1":                              # 1x1: identity, no table
        v = V(n_pad, n, n, 1, 1, 0, 0, 0)
        return 1, v, v
    if kind == "k3":                              # 3^3 stride 1: nbr + mask64 + out_row
        v = V(n_pad, n, n, 27, 27, 1, 0, 1)
        return 3, v, v
    assert kind == "k2"                           # 2^3 stride 2: n_pad of the COARSE map; four fine rows per coarse row
    n_fine = 4 * n
    if n_fine == 0:
        return 2, V(n_pad, 0, 0, 8, 8, 0, 0, 0), V(0, 0, 0, 1, 8, 0, 0, 0)
    gp = (n_fine + 8 * 256 + 255) // 256 * 256    # grouped fine view: eight groups, each padded to whole tiles
    return 2, V(n_pad, n_fine, n, 8, 8, 1, 0, 0), V(gp, n, n_fine, 1, 8, 1, 1, 1)


def sweep():
    """the pruned cross product, in a fixed order: -> [(knob, value, kind, n_pad, cin, cout, dtype, op, transposed, epilogue)]"""
    rows = []
    for kind, shapes in (("k1", SHAPES_K1), ("k3", SHAPES_K3), ("k2", SHAPES_K2)):
        for i, (cin, cout) in enumerate(shapes + SHAPES_ODD):
            probe, odd = i < 2, i >= len(shapes)                    # two model shapes per kind walk every map size
            for n_pad in (N_PADS if probe else [4096, 1200128] if odd else [19712, 1200128]):
                for dtype in (BF16, F32):
                    if dtype == F32 and not (probe or i % 3 == 0):
                        continue
                    for op in (0, 1):
                        for tr in ((0, 1) if kind == "k2" else (0,)):
                            if tr and not (probe or n_pad == 1200128):
                                continue
                            rows.append(("", 0, kind, n_pad, cin, cout, dtype, op, tr, 0))
                            if n_pad in (19712, 1200128) and (dtype == BF16 or probe) and not odd:
                                rows.append(("", 0, kind, n_pad, cin, cout, dtype, op, tr, 1 if op == 0 else 2))
    knob_cases = [("k3", s, n) for s in ((64, 64), (32, 64), (256, 256), (128, 96), (32, 32)) for n in (4096, 19712, 1200128)] + \
                 [("k1", s, n) for s in ((96, 200), (128, 96), (512, 512), (128, 128), (200, 96)) for n in (19712, 1200128)] + \
                 [("k2", (64, 64), 16384), ("k2", (256, 256), 4096)]
    for knob, value in KNOBS:
        for kind, (cin, cout), n_pad in knob_cases:
            for dtype in ((BF16, F32) if knob in ("FP32_SPLIT", "POINTWISE", "CONV_SPLIT") else (BF16,)):
                for op in ((0, 1) if cin != cout else (0,)):
                    rows.append((knob, value, kind, n_pad, cin, cout, dtype, op, 0, 0))
    return rows


def ask(views, op, tr, cin, cout, dtype, epi):
    from languagegroundedsemseg_amd import engine
    ks, fwd, bwd = views
    q = engine.ConvPlanQuery(fwd, bwd, ks, op, tr, cin, cout, dtype, epi)
    info = engine.ConvPlanInfo()
    engine.check(engine.lib().lgs_debug_conv_plan(ctypes.byref(q), ctypes.byref(info)))
    return info


def query(row):
    """one sweep row, under its knob -> (the dict of COLS as the library answers now, the plan, the plans of the other view / epilogue)"""
    from languagegroundedsemseg_amd import engine
    knob, value, kind, n_pad, cin, cout, dtype, op, tr, epi = row
    views = make_views(kind, n_pad)
    with engine.tuning(**({knob: value} if knob else {})):
        info = ask(views, op, tr, cin, cout, dtype, epi)
        others = [ask(views, op, t, cin, cout, dtype, e) for t in ((0, 1) if kind == "k2" else (0,)) for e in (0, 1 if op == 0 else 2)]
    out = dict(zip(QUERY_COLS, row))
    for c in EQUAL_COLS + INFO_COLS + ["workspace_bytes"]:
        out[c] = getattr(info.pack_desc, c[3:]) if c.startswith("pd_") else getattr(info, c)
    return out, info, others


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
    assert len(table) == len(want) and 300 <= len(want) <= 1500
    for rec, row in zip(table, want):
        assert tuple(rec[c] for c in QUERY_COLS) == tuple(row)


def test_table_covers_every_path(table):
    """every tile id, both pointwise paths, split and non-split 27-offset launches, the padded-input and scratch-output routes"""
    gather = [r for r in table if PATHS[r["path"]] == "gather"]
    assert {r["tile_id"] for r in gather} == set(range(0, 14)) | {16}
    assert any(PATHS[r["path"]] == "wide" and r["tile_id"] == 17 for r in table)
    for p in ("empty", "pointwise", "pointwise_f32"):
        assert any(PATHS[r["path"]] == p for r in table), p
    k3 = [r for r in gather if r["kind"] == "k3"]
    assert any(r["split"] == 1 and r["grid_z"] == 3 for r in k3) and any(r["split"] == 0 and r["grid_z"] == 1 for r in k3)
    assert any(r["pad_input"] for r in gather) and any(r["scratch_out"] for r in gather)
    assert any(r["pad_input"] and r["scratch_out"] for r in gather)
    assert any(r["q_bn_partial_rows"] > 0 for r in table) and any(r["q_can_accumulate"] for r in table)
    assert any(r["dtype"] == F32 and r["pd_dtype"] == 2 for r in table)                                  # split-fp32 image
    assert any(r["dtype"] == F32 and r["pd_dtype"] == F32 and r["pd_bytes"] for r in table)            # exact-fp32 image


def test_plan_equals_the_recorded_decisions(answers, table):
    assert len(answers) == len(table)
    for (got, _, _), rec in zip(answers, table):
        for c in EQUAL_COLS:
            assert got[c] == rec[c], "%s: %s = %s, recorded %s" % ({k: rec[k] for k in QUERY_COLS}, c, got[c], rec[c])


def test_workspace_does_not_grow(answers, table):
    for (got, _, _), rec in zip(answers, table):
        assert 0 < got["workspace_bytes"] <= rec["workspace_bytes"], ({k: rec[k] for k in QUERY_COLS}, got["workspace_bytes"], rec["workspace_bytes"])


def test_workspace_layout_is_sound(answers):
    """independent of the table: aligned, disjoint regions inside what lgs_conv_workspace_bytes reports for the map"""
    for got, info, others in answers:
        where = {k: got[k] for k in QUERY_COLS}
        ws = info.workspace_bytes
        used = [(n, getattr(info, n).offset, getattr(info, n).bytes) for n in ("packed", "padded_in", "scratch", "bias", "partials")]
        used = sorted((r for r in used if r[2] > 0), key=lambda r: r[1])
        for n, o, b in used:
            assert o % 256 == 0 and o >= 0, (where, n, o)
            assert o + b <= info.bytes_total <= ws, (where, n, o, b, info.bytes_total, ws)
        for (n0, o0, b0), (n1, o1, b1) in zip(used, used[1:]):
            assert o0 + b0 <= o1, (where, n0, n1)
        if PATHS[info.path] in ("gather", "wide"):
            assert info.total > 0 and info.total * 16 <= info.packed.bytes, (where, info.total * 16, info.packed.bytes)
            assert info.ncp >= info.nc and info.nbp >= info.nb_total and info.ncp % info.sc == 0 and info.nbp % info.wb == 0, where
            assert bool(info.padded_in.bytes) == bool(info.pad_input) and bool(info.scratch.bytes) == bool(info.scratch_out), where
            assert bool(info.partials.bytes) == bool(info.split), where
        # the map-level query covers the plan of either view under every epilogue (the caller sizes one buffer per map and shape)
        for other in others:
            assert other.workspace_bytes == ws and other.bytes_total <= ws, (where, other.bytes_total, ws)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        sys.path.insert(0, ROOT)
        rows = [[got[c] for c in COLS] for got, _, _ in map(query, sweep())]
        with open(TABLE, "w") as f:
            f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(COLS), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
        print("recorded", len(rows), "rows")
