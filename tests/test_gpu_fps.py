"""Furthest point sampling on the device (csrc/lgs_fps.hip, languagegroundedsemseg_amd/annotation.py) against the numpy restatement of
the contract (tests/fps_reference.py): exact equality of every index and every rank, in every tier and at every tier boundary."""
import functools

import numpy as np
import pytest
import torch

import fps_reference as fr
from languagegroundedsemseg_amd import annotation

pytestmark = [pytest.mark.gpu, pytest.mark.parity("the numpy restatement of the contract, tests/fps_reference.py")]

DEV = "cuda"
SIZES = [0, 1, 2, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1025] + \
        [b + d for b in annotation.TIER_BOUNDS for d in (-1, 0, 1)]
KINDS = 7          # 0, 1, 2, n - 1, n, n + 3, the 5 % rule


def count_of(kind, n):
    return [0, 1, 2, max(n - 1, 0), n, n + 3, fr.count_rule(n, 0.05)][kind % KINDS]


@functools.lru_cache(maxsize=None)
def main_points():
    """the segments of the main case, one after the other: random fp32, one exact-origin point and one point inside the 1e-3 ball"""
    rs = np.random.RandomState(11)
    parts = []
    for n in SIZES:
        p = rs.uniform(-4, 4, size=(n, 3)).astype(np.float32)
        if n >= 1:
            p[n // 3] = 0
        if n >= 2:
            p[n // 2 if n // 2 != n // 3 else n - 1] = (0.01, 0.02, 0.01)
        parts.append(p)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return np.concatenate(parts), off


_REFERENCE = {}


def main_reference(q, skip_origin, m=None):
    """the restatement's picks of segment q, computed once and shared: a run with fewer samples is a prefix of a longer one by
    construction, so a request is served from the longest run so far (n + 3 samples as soon as more than n / 2 are asked for)"""
    n = SIZES[q]
    m = n + 3 if m is None or 2 * m > n else m
    have = _REFERENCE.get((q, skip_origin))
    if have is None or len(have) < min(m, n + 3 if n else 0):
        p, off = main_points()
        have = fr.fps_contract(p[off[q]:off[q + 1]], m, skip_origin)
        have.setflags(write=False)
        _REFERENCE[(q, skip_origin)] = have
    return have


def expected(counts, skip_origin):
    p, off = main_points()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.zeros(starts[-1], dtype=np.int32)
    rank = np.full(p.shape[0], -1, dtype=np.int32)
    for q, m in enumerate(counts):
        out = main_reference(q, skip_origin, m)[:m if SIZES[q] else 0]
        idx[starts[q]:starts[q] + len(out)] = out
        first, where = np.unique(out, return_index=True)
        rank[off[q] + first] = where
    return idx, starts, rank


def run(points, off, counts, through=None, skip_origin=True):
    """one lgs_fps_segments call with both outputs -> (idx, rank) on the host"""
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = torch.from_numpy(np.ascontiguousarray(points)).to(DEV)
    idx = torch.zeros(int(starts[-1]), dtype=torch.int32, device=DEV)
    rank = torch.full((points.shape[0],), -7, dtype=torch.int32, device=DEV)
    annotation._fps_call(pts, None if through is None else torch.from_numpy(through).to(DEV), torch.from_numpy(np.asarray(off)).to(DEV),
                         counts=torch.tensor(list(counts), dtype=torch.int32).to(DEV), skip_origin=skip_origin,
                         out_offsets=torch.from_numpy(starts).to(DEV), idx_out=idx, rank_out=rank)
    return idx.cpu().numpy(), rank.cpu().numpy()


@pytest.mark.parametrize("skip_origin", [True, False])
def test_every_tier_and_boundary_equals_the_restatement(skip_origin):
    p, off = main_points()
    counts = [count_of(q, n) for q, n in enumerate(SIZES)]
    assert {q % KINDS for q in range(len(SIZES))} == set(range(KINDS))
    idx, rank = run(p, off, counts, skip_origin=skip_origin)
    want_idx, _, want_rank = expected(counts, skip_origin)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(rank, want_rank)
    if skip_origin:      # the near-origin points are never picked after round 0
        for q, n in enumerate(SIZES):
            if n >= 3:
                assert n // 3 not in main_reference(q, True, counts[q])[1:]


def test_shuffled_counts_give_each_segment_the_same_result_for_the_same_count():
    """the winner of a round is a function of the segment alone: with other counts next to it (other tiers busy, other workgroups
    running longer) a segment's picks are the same prefix"""
    p, off = main_points()
    first = [count_of(q, n) for q, n in enumerate(SIZES)]
    second = [count_of(q + 3, n) for q, n in enumerate(SIZES)]
    assert first != second
    idx1, _ = run(p, off, first)
    idx2, rank2 = run(p, off, second)
    want_idx, starts2, want_rank = expected(second, True)
    assert np.array_equal(idx2, want_idx) and np.array_equal(rank2, want_rank)
    starts1 = np.concatenate([[0], np.cumsum(first)])
    for q, n in enumerate(SIZES):
        both = min(first[q], second[q]) if n else 0
        assert np.array_equal(idx1[starts1[q]:starts1[q] + both], idx2[starts2[q]:starts2[q] + both]), q


def test_the_ratio_form_counts_on_the_device():
    p, off = main_points()
    rank = annotation.furthest_point_sample_segments(torch.from_numpy(p).to(DEV), torch.from_numpy(off).to(DEV), ratio=0.05)
    _, _, want = expected([fr.count_rule(n, 0.05) for n in SIZES], True)
    assert rank.dtype == torch.int32 and np.array_equal(rank.cpu().numpy(), want)
    # round-half-even and the minimum, where no segment of the main case meets them: 0.125 * 44 = 5.5 -> 6, 0.125 * 20 = 2.5 -> 5
    sizes = [44, 20, 100, 0, 52]
    o = np.concatenate([[0], np.cumsum(sizes)])
    q = np.random.RandomState(2).uniform(1, 3, size=(o[-1], 3)).astype(np.float32)
    rank = annotation.furthest_point_sample_segments(torch.from_numpy(q).to(DEV), o.tolist(), ratio=0.125).cpu().numpy()
    assert [int((rank[a:b] >= 0).sum()) for a, b in zip(o, o[1:])] == [6, 5, 12, 0, 6]
    assert np.array_equal(rank, fr.segments_contract(q, o, [fr.count_rule(n, 0.125) for n in sizes])[1])


def test_public_csr_form_and_offset_clamping():
    rs = np.random.RandomState(4)
    p = rs.uniform(-2, 2, size=(12, 3)).astype(np.float32)
    off = [-5, 3, 2, 10, 99]                     # clamped: [0, 3, 3, 10, 12]
    counts = [4, 2, 9, 1]
    idx, out_offsets = annotation.furthest_point_sample_segments(torch.from_numpy(p).to(DEV), off, counts=counts)
    want, _ = fr.segments_contract(p, off, counts)
    assert list(out_offsets.cpu().numpy()) == [0, 4, 6, 15, 16] and [len(w) for w in want] == [4, 0, 9, 1]
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, np.concatenate([want[0], [0, 0], want[2], want[3]]))


def test_one_large_segment():
    p = np.random.RandomState(7).uniform(-5, 5, size=(70000, 3)).astype(np.float32)
    got = annotation.furthest_point_sample(torch.from_numpy(p).to(DEV)[None], 3500)
    assert got.shape == (1, 3500) and got.dtype == torch.int32
    assert np.array_equal(got[0].cpu().numpy(), fr.fps_contract(p, 3500))


def test_ties_go_to_the_smallest_index():
    """a 2 cm grid in every tier (many exact ties) and segments of identical points"""
    parts, counts = [], []
    for side in (6, 12, 18, 21):
        g = np.arange(side, dtype=np.float32) * np.float32(0.02) + np.float32(1)
        parts.append(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
        counts.append(150)
    assert fr.fps_contract(parts[0], 150, return_ties=True)[1]
    for n in (100, 300):
        parts.append(np.zeros((n, 3), dtype=np.float32) + np.float32(1.5))
        counts.append(n + 3)
    parts.append(np.zeros((40, 3), dtype=np.float32))          # no eligible point at all
    counts.append(43)
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    p = np.concatenate(parts)
    idx, rank = run(p, off, counts)
    want, want_rank = fr.segments_contract(p, off, counts)
    assert np.array_equal(idx, np.concatenate(want)) and np.array_equal(rank, want_rank)
    assert not idx[-43 - 303 - 103:].any()


def test_through_gives_the_picks_of_the_gathered_copy():
    p, off = main_points()
    counts = [count_of(q + 6, n) for q, n in enumerate(SIZES)]
    through = np.random.RandomState(9).permutation(p.shape[0]).astype(np.int64)
    idx_a, rank_a = run(p[through], off, counts)
    idx_b, rank_b = run(p, off, counts, through=through)
    assert np.array_equal(idx_a, idx_b)
    assert np.array_equal(rank_b[through], rank_a) and (rank_a >= 0).sum() > 1000


def test_batched_form_equals_separate_calls():
    xyz = torch.from_numpy(np.random.RandomState(12).uniform(-1, 1, size=(3, 300, 3)).astype(np.float32)).to(DEV)
    got = annotation.furthest_point_sample(xyz, 40)
    assert got.shape == (3, 40) and got.dtype == torch.int32 and got.device == xyz.device
    for b in range(3):
        assert torch.equal(got[b], annotation.furthest_point_sample(xyz[b:b + 1], 40)[0])
        assert np.array_equal(got[b].cpu().numpy(), fr.fps_contract(xyz[b].cpu().numpy(), 40))
    assert annotation.furthest_point_sample(xyz, 0).shape == (3, 0)


def test_limited_annotation_equals_the_restatement_and_never_synchronises():
    p, ids, labels, off = fr.annotation_batch(big=2100)          # ids -1, an empty scene, an instance of 3 points, one above a tier bound
    want = fr.limited_annotation_contract(p, ids, labels, off, 0.05)
    args = [torch.from_numpy(a).to(DEV) for a in (p, ids, labels)] + [torch.tensor(off).to(DEV)]
    annotation.limited_annotation(*args, 0.05)                   # (the first call sizes the scratch buffers)
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = annotation.limited_annotation(*args, 0.05)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    assert got[1].dtype == torch.bool and got[2].dtype == torch.int32
    assert int(got[1].sum()) == int(want[1].sum()) > 100 and want[1][[3, 50, 88]].all()
    other = annotation.limited_annotation(*args, 0.05, unannotated_label=255, skip_origin=False)
    want = fr.limited_annotation_contract(p, ids, labels, off, 0.05, unannotated_label=255, skip_origin=False)
    assert np.array_equal(other[0].cpu().numpy(), want[0])


def test_two_calls_give_identical_bits():
    p, off = main_points()
    counts = [count_of(q + 3, n) for q, n in enumerate(SIZES)]
    a, b = run(p, off, counts), run(p, off, counts)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_knob_selects_the_torch_lines(monkeypatch):
    p = torch.from_numpy(np.random.RandomState(13).uniform(-1, 1, size=(2, 90, 3)).astype(np.float32)).to(DEV)
    fused = annotation.furthest_point_sample(p, 12)
    monkeypatch.setenv("LGS_FPS_FUSED", "0")
    assert torch.equal(annotation.furthest_point_sample(p, 12), fused)


def test_non_finite_coordinates_stay_in_bounds():
    p = np.random.RandomState(14).uniform(-1, 1, size=(700, 3)).astype(np.float32)
    p[5] = np.nan
    p[300, 1] = np.inf
    p[650] = -np.inf
    idx, rank = run(p, [0, 200, 700], [50, 120])
    assert idx.min() >= 0 and idx[:50].max() < 200 and idx[50:].max() < 500
    assert ((rank >= -1) & (rank < 120)).all()
