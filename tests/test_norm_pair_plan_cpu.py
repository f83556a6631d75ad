"""The launch plan of a pair of norms on the same rows (lgs_bn_forward_pair / lgs_bn_backward_pair, csrc/lgs_norm.hip), held on the
CPU through lgs_debug_norm_pair_plan: no HIP call, the one device query (co-resident workgroups of a grid-barrier kernel) is part
of the question, as for lgs_debug_norm_plan.

The pair derives everything from the SINGLE-norm plan of (direction, n, c, dtype): it takes today's two single calls (path 0)
exactly when that plan says `fused` (or the knob BN_PAIR is 0, or the tensor is empty), else the single plan's path with the
single plan's grids -- 3 launches (`three`) or 2 (`fold`) per direction -- and two sets of partial rows / `sums` rows behind one
another, aligned, disjoint and inside lgs_bn_pair_workspace_bytes(n, c), which may depend on neither knobs, dtype nor direction.
The recorded single-norm table (tests/test_norm_plan_cpu.py) is untouched by all this.
"""
import ctypes

import pytest

F32, BF16 = 0, 1
FWD, BWD = 0, 1
FOLD, FUSED, THREE = 1, 2, 3
NS = [0, 1, 127, 128, 129, 1037, 5000, 16383, 19648, 65536, 70001, 81920, 327583, 1205389, 600000000]
SHAPES = [(32, BF16), (32, F32), (96, BF16), (96, F32), (256, BF16), (2048, BF16)]
CAPS = [0, 15, 16, 256, 1024]
KNOBS = [("", 0), ("BN_FOLD", 0), ("BN_FOLD_MAX_MB", 64), ("BN_FOLD_PARTS", 1), ("BN_FOLD_GRID", 1), ("BN_FUSED", 0),
         ("BN_FUSED_MAX_MB", 64), ("BN_FUSED_FWD_MAX_MB", 24), ("BN_FUSED_BLOCKS", 64)]
REGIONS = ("partials_a", "partials_b", "sums_a", "sums_b")


@pytest.fixture(scope="module")
def eng():
    from languagegroundedsemseg_amd import engine
    engine.lib()
    return engine


def plans(engine, d, n, c, dt, cap):
    L = engine.lib()
    q = engine.NormPlanQuery(direction=d, c=c, dtype=dt, conv_partial_rows=0, resident_cap=cap, n=n)
    single, pair = engine.NormPlanInfo(), engine.NormPairPlanInfo()
    engine.check(L.lgs_debug_norm_plan(ctypes.byref(q), ctypes.byref(single)))
    engine.check(L.lgs_debug_norm_pair_plan(ctypes.byref(q), ctypes.byref(pair)))
    return single, pair


def sweep(engine):
    for knob, value in KNOBS:
        ctx = engine.tuning(**{knob: value}) if knob else engine.tuning()
        with ctx:
            for d in (FWD, BWD):
                for n in NS:
                    for c, dt in SHAPES:
                        for cap in (CAPS if not knob else [256]):
                            yield (knob, value, d, n, c, dt, cap), plans(engine, d, n, c, dt, cap)


def test_pair_follows_the_single_plan_and_counts_its_launches(eng):
    seen = set()
    for key, (single, pair) in sweep(eng):
        n = key[3]
        assert pair.single_path == single.path, key
        if single.path == FUSED or n == 0:
            assert pair.path == 0, key                        # today's two single calls
            continue
        assert pair.path == single.path and pair.path in (FOLD, THREE), key
        assert pair.launches == (3 if pair.path == THREE else 2), key
        # the single plan's grids: the same rows -> workgroup split, hence the same summation order per norm
        for f in ("reduce_grid", "rows_per_block", "fold_rows", "fold_grid", "apply_grid"):
            assert getattr(pair, f) == getattr(single, f), (key, f)
        seen.add((key[2], pair.path))
    assert seen == {(FWD, FOLD), (FWD, THREE), (BWD, FOLD), (BWD, THREE)}, seen


def test_pair_takes_single_calls_exactly_when_the_single_plan_is_fused(eng):
    fused = other = 0
    for key, (single, pair) in sweep(eng):
        if key[3] == 0:
            continue
        assert (pair.path == 0) == (single.path == FUSED), key
        fused += single.path == FUSED
        other += single.path != FUSED
    assert fused > 20 and other > 20, (fused, other)


def test_pair_workspace_regions_are_aligned_disjoint_and_inside_the_reported_size(eng):
    L = eng.lib()
    for key, (single, pair) in sweep(eng):
        _, _, d, n, c, dt, _ = key
        assert pair.workspace_bytes == L.lgs_bn_pair_workspace_bytes(n, c), key       # no knob, dtype or direction in it
        assert pair.workspace_bytes >= L.lgs_bn_workspace_bytes(n, c), key            # path 0 hands it to the single calls
        if pair.path == 0:
            assert pair.bytes_total == 0, key
            continue
        row = 4 * 2 * c
        regs = [(name, getattr(pair, name)) for name in REGIONS]
        assert pair.partials_a.bytes == pair.partials_b.bytes == row * pair.fold_rows, key
        want_sums = row if (d == BWD and pair.path == THREE) else 0
        assert pair.sums_a.bytes == pair.sums_b.bytes == want_sums, key
        end = 0
        for name, r in regs:
            if r.bytes == 0:
                continue
            assert r.offset % 16 == 0, (key, name)                                    # 16-byte accesses stay possible
            assert r.offset >= end, (key, name)                                       # behind one another: disjoint
            end = r.offset + r.bytes
        assert end == pair.bytes_total <= pair.workspace_bytes, key


def test_knob_off_restores_the_single_calls(eng):
    with eng.tuning(BN_PAIR=0):
        for d in (FWD, BWD):
            for n in (1, 5000, 81920, 1205389):
                single, pair = plans(eng, d, n, 96, BF16, 256)
                assert pair.path == 0 and pair.single_path == single.path
                assert pair.launches == 2 * {FOLD: 2, FUSED: 1, THREE: 3}[single.path]
    assert eng.tuning_get("BN_PAIR") == 1                    # the default is on

