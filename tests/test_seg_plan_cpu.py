"""CPU-side checks of the pooling / broadcast host plan (lgs_debug_seg_plan, csrc/lgs_pool.hip seg_plan): access width, lanes per
row, grids and the two-pass workspace layout over a small query space, against the contract of include/lgs_engine.h and
csrc/lgs_rows.h restated here (not by asking the library twice)."""
import ctypes
import itertools

FAMILIES = (0, 1, 2)          # lgs_seg_reduce, lgs_seg_broadcast, lgs_seg_max_backward


def _plan(**kw):
    from languagegroundedsemseg_amd import engine
    q = engine.SegPlanQuery(**kw)
    info = engine.SegPlanInfo()
    engine.check(engine.lib().lgs_debug_seg_plan(ctypes.byref(q), ctypes.byref(info)))
    return info


def _lanes_log2(c, per_lane):
    """the smallest lg <= 6 with 2^lg >= ceil(c / per_lane)"""
    chunks = -(-c // per_lane)
    return next((lg for lg in range(7) if (1 << lg) >= chunks), 6)


def _grid(units, lg):
    return max(1, -(-(units << lg) // 256))


def test_plan_width_lanes_grids_and_workspace():
    from languagegroundedsemseg_amd import engine
    a256 = lambda b: (b + 255) // 256 * 256
    space = itertools.product(FAMILIES, (3, 8, 20, 96, 200, 512), (engine.LGS_F32, engine.LGS_BF16), (0, 1), (0, 1), (0, 1, 7, 3000),
                              (0, 1, 5, 40000))
    seen = 0
    for family, c, dtype, vec_ok, single, n_items, n_coarse in space:
        n_fine = 3 * n_coarse + 1 if n_coarse else 0
        p = _plan(family=family, c=c, dtype=dtype, single_pass=single, vec_ok=vec_ok, n_fine=n_fine, n_coarse=n_coarse, n_items=n_items)
        what = (family, c, dtype, vec_ok, single, n_items, n_coarse)
        es = 2 if dtype == engine.LGS_BF16 else 4
        assert p.vec == (1 if vec_ok and (c * es) % 16 == 0 else 0), what
        lg, lgc = _lanes_log2(c, 16 // es if p.vec else 1), _lanes_log2(c, 1)
        assert (p.lanes_log2, p.combine_lanes_log2) == (lg, lgc), what
        two_pass = family == 0 and not single
        want = {"reduce_grid": _grid(n_coarse if single else n_items, lg) if family == 0 else 0,
                "combine_grid": _grid(n_coarse, lgc) if two_pass else 0,
                "bcast_grid": _grid(n_fine, lg) if family == 1 else 0,
                "max_bwd_grid": _grid(n_fine, lg) if family == 2 else 0}
        assert {k: getattr(p, k) for k in want} == want, what
        # lgs_seg_workspace_bytes: of the map and c alone
        assert p.workspace_bytes == (0 if single else 2 * a256(n_items * c * 4)), what
        regions = (p.partials, p.partial_argmax)
        if not two_pass:
            assert p.bytes_total == 0 and all(r.offset == 0 and r.bytes == 0 for r in regions), what
        else:
            for r in regions:
                assert r.offset % 256 == 0 and r.bytes % 256 == 0 and r.bytes >= n_items * c * 4, what
            assert p.partials.offset == 0 and p.partial_argmax.offset == p.partials.offset + p.partials.bytes, what
            assert p.partial_argmax.offset + p.partial_argmax.bytes == p.bytes_total <= p.workspace_bytes, what
        seen += 1
    assert seen == 3 * 6 * 2 * 2 * 2 * 4 * 4


def test_plan_refuses_bad_queries():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    info = engine.SegPlanInfo()
    for kw in (dict(family=3, c=8, dtype=0), dict(family=0, c=0, dtype=0), dict(family=0, c=8, dtype=7), dict(family=1, c=8, dtype=0, n_items=-1)):
        q = engine.SegPlanQuery(**{**dict(n_fine=10, n_coarse=2, n_items=1, single_pass=0, vec_ok=1), **kw})
        assert L.lgs_debug_seg_plan(ctypes.byref(q), ctypes.byref(info)) != 0
        assert b"lgs_debug_seg_plan" in L.lgs_last_error()


def test_segment_map_caches_the_workspace_size_per_channel_count():
    """HipSegmentMap asks lgs_seg_workspace_bytes once per c (no knob feeds the answer)"""
    from languagegroundedsemseg_amd.me.backend_hip import HipSegmentMap

    class Mgr:
        def map_size(self, key):
            return 10

    class Lib:
        calls = []

        def lgs_seg_workspace_bytes(self, h, c):
            self.calls.append(c)
            return 512 * c

    sm, L = HipSegmentMap(Mgr(), None, 0, 1), Lib()
    assert [sm._ws_bytes(L, c) for c in (8, 8, 96, 8, 96)] == [4096, 4096, 49152, 4096, 49152]
    assert L.calls == [8, 96]
