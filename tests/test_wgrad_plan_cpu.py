"""The launch plan of the weight gradient (WgradPlan, csrc/lgs_wgrad.hip), held on the CPU through lgs_debug_wgrad_plan: no HIP
call, the kernel maps are synthetic.

tests/golden/wgrad_plan_table.json was recorded from the code BEFORE the plan existed, through a shim that walked the try-cascade
of lgs_conv_wgrad (conv_wgrad_wide -> padded conv_wgrad_ps -> conv_wgrad_ps -> conv_wgrad_bf16 / conv_wgrad_f32path, each with
its own plan and its own reasons to decline) without launching.  Every row must still give the same path, template parameters,
grid, LDS bytes, slots and public answers, and may not need a larger workspace.

Independently of the table, the workspace layout of every row must be sound: aligned, disjoint regions, each large enough for
what its kernel writes, inside the size lgs_conv_workspace_bytes(op 2) reports for the map -- whichever `transposed` / row
stride the caller then uses with that one buffer.

`python tests/test_wgrad_plan_cpu.py --record` rewrites the table from the library as built (only when a behaviour change is
intended).
"""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_plan_cpu import BF16, F32, N_PADS, SHAPES_K1, SHAPES_K2, SHAPES_K3, SHAPES_ODD, make_views   # noqa: E402  (the same maps and shapes)

TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_plan_table.json")
BIG = 4000000     # rows x 544 channels of bf16 pass 4 GiB, rows x 512 do not: the descriptor-limit branches
KNOBS = [("WGRAD_WIDE", 0), ("WW_MIN_ROWS", 0), ("WW_RANGE", 8192), ("WW_RANGE", 32768), ("WW_RANGE", 65536), ("WGRAD_PS", 0), ("PS_WIDE3", 0),
         ("PS_CUS", 8), ("PS_CUS", 32), ("WGRAD_F32_LDS", 0), ("WGRAD_F32_LDS", 1), ("WGRAD_F32_LDS", 3)]
PATHS = {0: "empty", 1: "wide", 2: "ps", 3: "pairs", 4: "f32"}
K_OF = {"k1": 1, "k3": 27, "k2": 8}

QUERY_COLS = ["knob", "knob_value", "kind", "n_pad", "cin", "cout", "dtype", "transposed", "in_row_stride"]
EQUAL_COLS = ["path", "bwd_view", "in_place", "pad_in", "pad_gout", "all_cus", "f32_kernel", "t0", "t1", "pad_a", "pad_b", "slots", "span",
              "n_ranges", "kpw", "tasks_a", "tasks_b", "cpl", "n_chunks", "xcd_map", "ntile", "grid_x", "grid_y", "grid_z", "lds_bytes",
              "reduce_blocks"]
COLS = QUERY_COLS + EQUAL_COLS + ["supports_stride", "workspace_bytes"]
REGIONS = ("partials", "padded_in", "padded_gout", "ww_count", "ww_offset", "ww_total", "ww_pair_in", "ww_pair_out")

# tests/golden/wgrad_plan_stride_changed.json lists the rows whose recorded lgs_conv_wgrad_supports_stride differs from the plan's.
# The old function mirrored conv_wgrad_ps by hand and was wrong about what lgs_conv_wgrad then did, in three ways:
#  "copy":    it answered 1 to every stride-less query (in_row_stride 0 or cin) of a bf16 2^3 / 3^3 map, also where no kernel that
#             can read a row stride serves the shape: the pair-list kernel or the zero-padded copy (odd widths, the 4 GiB and
#             partial-slab limits).  No caller asks without a stride; the answer now says what the kernel can do;
#  "wide":    with WGRAD_PS=0 it answered 0 although k_wgrad_wide serves the call and reads the stride in place;
#  "require": it tested the gathered operand's bytes and row grid only: 1 where both in-place kernels decline (a stationary
#             operand or neighbour table of >= 4 GiB, the stationary row grid) and the strided call then failed in lgs_conv_wgrad.
# Each listed row must answer "1 exactly when the planned kernel reads `in` in place"; every other row must equal the record.
STRIDE_ANSWER_CHANGED = os.path.join(ROOT, "tests", "golden", "wgrad_plan_stride_changed.json")


def changed_kind(rec):
    """why a listed row may differ from its record, from the RECORDED columns alone (None: it may not)"""
    stride_less = rec["in_row_stride"] in (0, rec["cin"])
    if rec["supports_stride"] == 1 and not rec["in_place"]:
        return "copy" if stride_less else "require"
    if rec["supports_stride"] == 0 and rec["in_place"] and rec["knob"] == "WGRAD_PS" and PATHS[rec["path"]] == "wide":
        return "wide"
    return None


def strides(cin):
    return [0, cin, 544 if cin == 512 else cin + 32, cin + 4]      # contiguous twice, a wider multiple of 8, off the 16-byte grid


def sweep():
    """the pruned cross product, in a fixed order: -> [(knob, value, kind, n_pad, cin, cout, dtype, transposed, in_row_stride)]"""
    rows = []
    for kind, shapes in (("k1", SHAPES_K1), ("k3", SHAPES_K3), ("k2", SHAPES_K2)):
        for i, (cin, cout) in enumerate(shapes + SHAPES_ODD):
            probe, odd = i < 2, i >= len(shapes)                    # two model shapes per kind walk every map size
            sizes = N_PADS if probe else [4096, 1200128] if odd else [19712, 1200128]
            if kind != "k1" and (probe or (cin, cout) in ((544, 512), (512, 512), (256, 512), (96, 96), (3, 32))):
                sizes = sizes + [BIG]
            for n_pad in sizes:
                for dtype in (BF16, F32):
                    if dtype == F32 and not (probe or odd or i % 3 == 0):
                        continue
                    for tr in ((0, 1) if kind == "k2" else (0,)):
                        wide = dtype == BF16 and n_pad in (19712, 1200128, BIG) and (kind != "k1" or probe)
                        for ld in (strides(cin) if wide else [0, cin + 32] if probe else [0]):
                            rows.append(("", 0, kind, n_pad, cin, cout, dtype, tr, ld))
    bf16_cases = [("k3", s, n) for s in ((64, 64), (256, 256), (512, 512), (544, 512), (128, 96), (3, 32), (96, 3), (384, 256))
                  for n in (19712, 81920, 1200128)] + \
                 [("k2", s, n) for s in ((64, 64), (256, 256), (256, 512)) for n in (16384, 1200128)] + [("k1", (512, 512), 1200128), ("k3", (512, 512), BIG)]
    f32_cases = [(k, s, n) for k in ("k1", "k3") for s in ((64, 64), (3, 32), (96, 96), (32, 64), (96, 200), (512, 200), (5, 64)) for n in (4096, 1200128)]
    for knob, value in KNOBS:
        f32 = knob == "WGRAD_F32_LDS"
        for kind, (cin, cout), n_pad in (f32_cases if f32 else bf16_cases):
            for tr in ((0, 1) if kind == "k2" else (0,)):
                for ld in ([0] if f32 else [0, 544 if cin == 512 else cin + 32]):
                    rows.append((knob, value, kind, n_pad, cin, cout, F32 if f32 else BF16, tr, ld))
    return rows


def ask(views, tr, cin, cout, dtype, ld):
    from languagegroundedsemseg_amd import engine
    ks, fwd, bwd = views
    q = engine.WgradPlanQuery(fwd, bwd, ks, tr, cin, cout, dtype, ld)
    info = engine.WgradPlanInfo()
    engine.check(engine.lib().lgs_debug_wgrad_plan(ctypes.byref(q), ctypes.byref(info)))
    return info


def launchable(info, cin, ld):
    """a strided call is only made where the kernel reads the stride in place (the caller asks first)"""
    return ld in (0, cin) or bool(info.in_place)


def query(row):
    """one sweep row, under its knob -> (the dict of COLS as the library answers now, the plan, the launchable plans of the other
    `transposed` / row-stride values on the same map)"""
    from languagegroundedsemseg_amd import engine
    knob, value, kind, n_pad, cin, cout, dtype, tr, ld = row
    views = make_views(kind, n_pad)
    with engine.tuning(**({knob: value} if knob else {})):
        info = ask(views, tr, cin, cout, dtype, ld)
        calls = [(t, s) for t in ((0, 1) if kind == "k2" else (0,)) for s in (strides(cin) if dtype == BF16 else [0])]
        others = [o for o, (t, s) in ((ask(views, t, cin, cout, dtype, s), (t, s)) for t, s in calls) if launchable(o, cin, s)]
    out = dict(zip(QUERY_COLS, row))
    for c in EQUAL_COLS + ["supports_stride", "workspace_bytes"]:
        out[c] = getattr(info, c)
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


@pytest.fixture(scope="module")
def stride_changed():
    t = json.load(open(STRIDE_ANSWER_CHANGED))
    assert t["columns"] == QUERY_COLS
    return {tuple(r) for r in t["rows"]}


def test_table_is_the_sweep(table):
    want = sweep()
    assert len(table) == len(want) and 300 <= len(want) <= 3000
    assert os.path.getsize(TABLE) < (1 << 20)
    for rec, row in zip(table, want):
        assert tuple(rec[c] for c in QUERY_COLS) == tuple(row)


def test_table_covers_every_path(table):
    """every kernel family and every route into it, and every reason a kernel declines a call"""
    def rows(path, **kw):
        return [r for r in table if PATHS[r["path"]] == path and all(r[k] == v for k, v in kw.items())]
    assert rows("empty") and rows("wide", in_place=1)
    assert any(r["in_row_stride"] not in (0, r["cin"]) for r in rows("wide")), "k_wgrad_wide on a strided input"
    ps = rows("ps")
    assert {(r["t0"], r["t1"]) for r in ps} == {(27, 1), (27, 2), (27, 3), (8, 1), (8, 2), (8, 3), (8, 4)}
    assert rows("ps", pad_in=8, all_cus=1, in_place=0) and rows("ps", transposed=1, in_place=1) and rows("ps", xcd_map=0) and rows("ps", xcd_map=1)
    assert any(r["in_row_stride"] not in (0, r["cin"]) for r in ps), "k_wgrad_ps on a strided input"
    pairs = rows("pairs")
    assert len({(r["t0"], r["t1"]) for r in pairs}) >= 8 and {r["kpw"] for r in pairs} == {1, 4}
    assert any(r["pad_in"] and not r["pad_gout"] for r in pairs) and any(r["pad_gout"] and not r["pad_in"] for r in pairs)
    assert any(r["pad_in"] and r["pad_gout"] for r in pairs) and rows("pairs", bwd_view=1)
    f32 = rows("f32")
    assert {r["f32_kernel"] for r in f32} == {0, 1, 2} and {r["t0"] for r in f32} == {1, 2, 3, 4}
    assert any(r["pad_in"] == 4 for r in f32) and any(r["cin"] % 4 and not r["pad_in"] for r in f32)
    # the knobs at work: each changes the decision of at least one row against the same query without it
    base = {tuple(r[c] for c in QUERY_COLS[2:]): r for r in table if not r["knob"]}
    for knob, value in KNOBS:
        changed = 0
        for r in table:
            b = base.get(tuple(r[c] for c in QUERY_COLS[2:]))
            if (r["knob"], r["knob_value"]) == (knob, value) and b is not None and any(r[c] != b[c] for c in EQUAL_COLS):
                changed += 1
        assert changed, (knob, value)
    # the declines: a strided tensor of >= 4 GiB and a row stride off the 16-byte grid leave wide / ps for the pair list (which cannot
    # serve the strided call: in_place 0), the partial-slab caps, WGRAD_PS / WGRAD_WIDE
    for path in ("wide", "ps"):
        took = {tuple(r[c] for c in QUERY_COLS[:8]) for r in rows(path, in_row_stride=0)}
        lost = [r for r in pairs if r["in_row_stride"] not in (0, r["cin"]) and tuple(r[c] for c in QUERY_COLS[:8]) in took]
        assert any(r["n_pad"] == BIG and r["in_row_stride"] % 8 == 0 for r in lost), path
        assert any(r["in_row_stride"] % 8 for r in lost), path
    assert any(r["n_pad"] == BIG for r in pairs if r["in_row_stride"] == 0 and r["kind"] != "k1" and r["cin"] % 8 == 0 and r["cout"] % 8 == 0)


def test_plan_equals_the_recorded_decisions(answers, table):
    assert len(answers) == len(table)
    for (got, _, _), rec in zip(answers, table):
        for c in EQUAL_COLS:
            assert got[c] == rec[c], "%s: %s = %s, recorded %s" % ({k: rec[k] for k in QUERY_COLS}, c, got[c], rec[c])


def test_workspace_does_not_grow(answers, table):
    for (got, _, _), rec in zip(answers, table):
        assert 0 < got["workspace_bytes"] <= rec["workspace_bytes"], ({k: rec[k] for k in QUERY_COLS}, got["workspace_bytes"], rec["workspace_bytes"])


def test_supports_stride(answers, table, stride_changed):
    seen = set()
    for (got, info, _), rec in zip(answers, table):
        key = tuple(rec[c] for c in QUERY_COLS)
        assert got["supports_stride"] == info.in_place, key          # 1 exactly when the planned kernel reads `in` in place
        if key in stride_changed:
            seen.add(key)
            assert got["supports_stride"] != rec["supports_stride"] and changed_kind(rec), ("listed without a reason", key)
        else:
            assert got["supports_stride"] == rec["supports_stride"], (key, got["supports_stride"], rec["supports_stride"])
    assert seen == stride_changed
    kinds = [changed_kind(rec) for rec in table if tuple(rec[c] for c in QUERY_COLS) in stride_changed]
    assert kinds.count("wide") <= 10 and kinds.count("require") <= 12, kinds      # the handful the mirror got wrong on strided calls


def test_workspace_layout_is_sound(answers):
    """independent of the table: aligned, disjoint regions that hold what the kernels write, inside what lgs_conv_workspace_bytes
    reports for the map"""
    for got, info, others in answers:
        where = {k: got[k] for k in QUERY_COLS}
        ws = info.workspace_bytes
        used = sorted(((n, getattr(info, n).offset, getattr(info, n).bytes) for n in REGIONS if getattr(info, n).bytes > 0), key=lambda r: r[1])
        for n, o, b in used:
            assert o % 256 == 0 and o >= 0, (where, n, o)
            assert o + b <= info.bytes_total, (where, n, o, b, info.bytes_total)
        assert info.bytes_total <= ws or not launchable(info, got["cin"], got["in_row_stride"]), (where, info.bytes_total, ws)
        for (n0, o0, b0), (n1, o1, b1) in zip(used, used[1:]):
            assert o0 + b0 <= o1, (where, n0, n1)
        path = PATHS[info.path]
        assert (path == "empty") == (not used), where
        if path == "empty":
            continue
        ks, fwd, bwd = make_views(got["kind"], got["n_pad"])
        view = bwd if info.bwd_view else fwd
        e = 2 if got["dtype"] == BF16 else 4
        slabs = 27 * info.slots if path == "wide" else info.slots * K_OF[got["kind"]]
        assert info.partials.bytes >= slabs * info.pad_a * info.pad_b * 4 > 0, (where, info.partials.bytes)
        assert bool(info.padded_in.bytes) == bool(info.pad_in) and bool(info.padded_gout.bytes) == bool(info.pad_gout), where
        assert info.padded_in.bytes >= view.n_in * info.pad_in * e and info.padded_gout.bytes >= view.n_out * info.pad_gout * e, where
        assert not info.pad_in or info.pad_in >= got["cin"]
        assert not info.pad_gout or info.pad_gout >= got["cout"]
        if path == "wide":
            assert info.ww_count.bytes >= 27 * info.ntile * 4 and info.ww_offset.bytes >= 27 * info.ntile * 4 and info.ww_total.bytes >= 27 * 4, where
            assert info.ww_pair_in.bytes >= 27 * view.n_pad * 4 and info.ww_pair_out.bytes >= 27 * view.n_pad * 4, where
            assert info.ntile * 256 == view.n_pad
        else:
            assert not any(getattr(info, n).bytes for n in REGIONS[3:]), where
        # one buffer per map and shape: the map-level query covers every call the caller can make with it
        for other in others:
            assert other.workspace_bytes == ws and other.bytes_total <= ws, (where, other.bytes_total, ws)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        sys.path.insert(0, ROOT)
        rows = [[got[c] for c in COLS] for got, _, _ in map(query, sweep())]
        with open(TABLE, "w") as f:
            f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(COLS), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
        print("recorded", len(rows), "rows")
