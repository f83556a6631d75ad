"""What a kernel-map request (in_key, out_key, kernel_size, dilation) names, held on the CPU through lgs_debug_kmap_relation: the
classifier and the trait table that both map entry points, the plans and the conv entry points read (csrc/lgs_common.h).

The expectation below is written out from the contract of include/lgs_engine.h (the comments of lgs_manager_kernel_map and
lgs_manager_kernel_map_ex), not read back from the library; the messages are the ones the entry points have always given, in the
order a caller meets them."""
import ctypes
import itertools

import pytest

OLD, EX = 0, 1
SAME, TO_COARSE, TO_FINE, UNRELATED = 0, 1, 2, 3
ENTRIES, KS, LINKS = (OLD, EX), (1, 2, 3, 5), (SAME, TO_COARSE, TO_FINE, UNRELATED)
DILATIONS, STRIDES = (0, 1, 2, 4, 1 << 17), (1, 2, 4096)
NAME = {OLD: "lgs_manager_kernel_map", EX: "lgs_manager_kernel_map_ex"}

# relation -> (id, kernel_size, K, strided, bwd_mirror, transposed_ok, served_by_old_entry): the six rows of the header
IDENTITY, CONV3, CONV2_S2, CONV3_DILATED, CONV3_S2, CONV1_S2 = range(6)
ROWS = {
    IDENTITY:      (1, 1, 0, 0, 1, 1),      # kernel_size 1, in_key == out_key
    CONV3:         (3, 27, 0, 1, 0, 1),     # kernel_size 3, in_key == out_key: the one map that refuses `transposed`
    CONV2_S2:      (2, 8, 1, 0, 1, 1),      # kernel_size 2, out_key == stride2(in_key); the transposed conv uses the same object
    CONV3_DILATED: (3, 27, 0, 1, 1, 0),     # kernel_size 3, in_key == out_key, dilation >= 2: bwd = fwd read mirrored
    CONV3_S2:      (3, 27, 1, 0, 1, 0),     # kernel_size 3, out_key == stride2(in_key): slot k = offset k on both views
    CONV1_S2:      (1, 1, 1, 0, 1, 0),      # kernel_size 1, out_key == stride2(in_key)
}
MSG_KS = {1: "kernel_size 1 needs in_key == out_key", 3: "kernel_size 3 is supported for stride 1 (in_key == out_key) only",
          2: "kernel_size 2 needs out_key == stride2(in_key)", 5: "unsupported kernel_size (the model family uses 1, 2 and 3 only)"}


def expected(entry, ks, link, dilation, ts, out_sorted, origin):
    """-> (relation, None) or (None, the message's fixed text)"""
    if origin:
        return None, NAME[entry] + ": no kernel maps on the origin map"
    if entry == OLD:           # three relations, no dilation argument, everything else refused
        rel = {(1, SAME): IDENTITY, (3, SAME): CONV3, (2, TO_COARSE): CONV2_S2}.get((ks, link))
        return (rel, None) if rel is not None else (None, MSG_KS[ks])
    ex = NAME[EX] + ": "
    if dilation < 1:
        return None, ex + "dilation must be >= 1"
    if dilation > 1:
        if link == TO_COARSE:
            return None, ex + "stride 2 combined with dilation > 1 is not supported"
        if ks != 3:
            return None, ex + "dilation > 1 needs kernel_size 3"
        if link != SAME:
            return None, ex + "out_key must be in_key or stride2(in_key)"
        rel = CONV3_DILATED
    else:
        rel = {(1, SAME): IDENTITY, (3, SAME): CONV3, (2, TO_COARSE): CONV2_S2, (3, TO_COARSE): CONV3_S2, (1, TO_COARSE): CONV1_S2}.get((ks, link))
        if rel is None:
            return None, MSG_KS[ks]
    if rel in (CONV3_S2, CONV1_S2) and not out_sorted:
        return None, ex + "the stride-2 map's rows are not in sorted order"
    if rel in (CONV3_DILATED, CONV3_S2, CONV1_S2) and dilation * ts >= 1 << 17:
        return None, ex + "dilation * tensor_stride must stay below 2^17"
    return rel, None


@pytest.fixture(scope="module")
def ask():
    from languagegroundedsemseg_amd import build, engine
    build.build()
    L = engine.lib()

    def ask(entry, ks, link, dilation=1, ts=1, out_sorted=1, in_origin=0, out_origin=0):
        q = engine.KmapRelationQuery(entry, ks, dilation, link, ts, out_sorted, in_origin, out_origin)
        info = engine.KmapRelationInfo()
        rc = L.lgs_debug_kmap_relation(ctypes.byref(q), ctypes.byref(info))
        assert rc == info.rc
        return info, (L.lgs_last_error().decode() if rc else None)
    return ask


def space():
    for entry, ks, link, d, ts, srt in itertools.product(ENTRIES, KS, LINKS, DILATIONS, STRIDES, (1, 0)):
        for io, oo in ((0, 0), (1, 0), (0, 1), (1, 1)):
            yield entry, ks, link, d, ts, srt, io, oo


def test_the_whole_query_space_against_the_contract(ask):
    accepted = set()
    for entry, ks, link, d, ts, srt, io, oo in space():
        where = (NAME[entry], ks, link, d, ts, srt, io, oo)
        want, msg = expected(entry, ks, link, d, ts, srt, io or oo)
        info, err = ask(entry, ks, link, d, ts, srt, io, oo)
        if want is None:
            assert info.rc == 2 and info.relation == -1 and err and err.startswith(msg), (where, info.rc, err, msg)
            assert (info.K, info.strided, info.bwd_mirror, info.transposed_ok, info.served_by_old_entry) == (0, 0, 0, 0, 0), where
            continue
        assert info.rc == 0 and info.relation == want, (where, info.rc, info.relation, err)
        k, K, strided, mirror, tr_ok, old = ROWS[want]
        assert k == ks and (info.K, info.strided, info.bwd_mirror, info.transposed_ok, info.served_by_old_entry) == (K, strided, mirror, tr_ok, old), where
        for tr in (0, 1):
            assert info.pairs_only[tr] == int(ks == 3 and bool(strided or tr)), (where, tr)
        accepted.add((entry, want))
    # the six rows are all reached through _ex, the old three through the old entry point, and nothing else is accepted
    assert accepted == {(EX, r) for r in ROWS} | {(OLD, r) for r in (IDENTITY, CONV3, CONV2_S2)}


def test_the_six_rows_and_their_traits(ask):
    for rel, (ks, link, d) in {IDENTITY: (1, SAME, 1), CONV3: (3, SAME, 1), CONV2_S2: (2, TO_COARSE, 1), CONV3_DILATED: (3, SAME, 2),
                               CONV3_S2: (3, TO_COARSE, 1), CONV1_S2: (1, TO_COARSE, 1)}.items():
        info, _ = ask(EX, ks, link, d)
        assert info.rc == 0 and info.relation == rel and info.K == ks ** 3
        # `transposed` is refused on the plain 3^3 stride-1 map and taken on every map that only _ex builds
        assert info.transposed_ok == (0 if rel == CONV3 else 1)
        assert info.served_by_old_entry == int(rel in (IDENTITY, CONV3, CONV2_S2))
        # the old entry point refuses exactly the relations that are _ex's alone (it has no dilation: it sees a dilated request as d = 1)
        old, err = ask(OLD, ks, link, d)
        if rel == CONV3_DILATED:
            assert old.rc == 0 and old.relation == CONV3
        else:
            assert (old.rc == 0) == bool(info.served_by_old_entry) and (old.rc == 0 or err), (rel, old.rc, err)
        # dilation 4 is a dilated map too; dilation 1 on the dilated row's keys is the plain map (the scale is data)
        if rel == CONV3_DILATED:
            assert ask(EX, 3, SAME, 4)[0].relation == CONV3_DILATED and ask(EX, 3, SAME, 1)[0].relation == CONV3


def test_the_refusals_of_the_gpu_test_are_refused_here(ask):
    """the list of tests/test_gpu_strided_conv.py::test_the_old_entry_point_and_the_cache_are_untouched, k0 a stride-1 map, k1 = stride2(k0)"""
    ex = NAME[EX] + ": "
    for (link, ks, d), msg in (((TO_COARSE, 3, 2), ex + "stride 2 combined with dilation > 1 is not supported"),
                               ((TO_COARSE, 1, 2), ex + "stride 2 combined with dilation > 1 is not supported"),
                               ((SAME, 1, 2), ex + "dilation > 1 needs kernel_size 3"),
                               ((SAME, 5, 1), MSG_KS[5]),
                               ((TO_FINE, 3, 1), MSG_KS[3]),
                               ((SAME, 3, 1 << 17), ex + "dilation * tensor_stride must stay below 2^17"),
                               ((SAME, 3, 0), ex + "dilation must be >= 1")):
        info, err = ask(EX, ks, link, d)
        assert info.rc != 0 and err and err.startswith(msg), (link, ks, d, err)
    info, err = ask(OLD, 3, TO_COARSE)          # "the old entry point keeps refusing the strided 3^3 relation"
    assert info.rc != 0 and err.startswith(MSG_KS[3])


def test_the_order_of_the_checks(ask):
    """origin before the dilation range, the range before stride-with-dilation, that before the kernel size"""
    ex = NAME[EX] + ": "
    assert ask(EX, 5, TO_COARSE, 0, in_origin=1)[1].startswith(ex + "no kernel maps on the origin map")
    assert ask(OLD, 5, UNRELATED, out_origin=1)[1].startswith(NAME[OLD] + ": no kernel maps on the origin map")
    assert ask(EX, 5, TO_COARSE, 0)[1].startswith(ex + "dilation must be >= 1")
    assert ask(EX, 5, TO_COARSE, 2)[1].startswith(ex + "stride 2 combined")
    assert ask(EX, 5, UNRELATED, 2)[1].startswith(ex + "dilation > 1 needs kernel_size 3")
    assert ask(EX, 3, UNRELATED, 2)[1].startswith(ex + "out_key must be in_key or stride2(in_key)")
    assert ask(EX, 3, TO_COARSE, 1, ts=4096, out_sorted=0)[1].startswith(ex + "the stride-2 map's rows are not in sorted order")
    # the old three relations never look at the tensor stride or the row order
    assert ask(EX, 2, TO_COARSE, 1, ts=4096, out_sorted=0)[0].rc == 0 and ask(EX, 3, SAME, 1, ts=1 << 20)[0].rc == 0
    assert ask(EX, 3, SAME, 4, ts=4096)[0].rc == 0 and ask(EX, 3, SAME, 32, ts=4096)[0].rc == 2


def test_a_malformed_query_is_an_error(ask):
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    info = engine.KmapRelationInfo()
    for q in (engine.KmapRelationQuery(2, 3, 1, SAME, 1, 1, 0, 0), engine.KmapRelationQuery(EX, 3, 1, 4, 1, 1, 0, 0)):
        assert L.lgs_debug_kmap_relation(ctypes.byref(q), ctypes.byref(info)) != 0 and b"lgs_debug_kmap_relation" in L.lgs_last_error()
    assert L.lgs_debug_kmap_relation(None, None) != 0
