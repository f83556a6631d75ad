"""Furthest point sampling without a GPU: the numpy restatement of the contract (tests/fps_reference.py) against a brute-force
definition and against the reference's kernel as it is written, the count rule, the C-ABI's size answers and refusals, and the torch
path of languagegroundedsemseg_amd/annotation.py on CPU tensors."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import fps_reference as fr
from languagegroundedsemseg_amd import annotation, engine, tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cloud(n, seed, origin_at=None):
    p = np.random.RandomState(seed).uniform(-3, 3, size=(n, 3)).astype(np.float32)
    if origin_at is not None:
        p[origin_at] = 0
    return p


def brute_force(p, m):
    """the definition: the next sample maximises the minimum distance to the chosen set, the smallest index on a tie (float64 on
    integer coordinates: exact)"""
    p = np.asarray(p, dtype=np.float64)
    out = [0]
    while len(out) < m:
        dmin = np.min(((p[:, None, :] - p[None, out, :]) ** 2).sum(-1), axis=1)
        out.append(int(np.argmax(dmin)))
    return np.array(out[:m], dtype=np.int32)


@pytest.mark.parametrize("n, seed", [(1, 0), (2, 1), (5, 2), (9, 3), (12, 4), (12, 5)])
def test_restatement_is_the_arg_max_of_the_minimum_distance(n, seed):
    p = np.random.RandomState(seed).randint(-20, 21, size=(n, 3)).astype(np.float32)
    for m in (1, n, n + 3):
        assert np.array_equal(fr.fps_contract(p, m, skip_origin=False), brute_force(p, m))


@pytest.mark.parametrize("n", [1, 4, 65, 700, 1300])
def test_contract_equals_the_kernel_as_written_on_tie_free_clouds(n):
    p = cloud(n, 100 + n, origin_at=n // 2)
    m = max(n - 1, 1)                        # every eligible point once: no round after exhaustion
    assert fr.tie_free(p, m)
    want = fr.fps_contract(p, m)
    assert n == 1 or n // 2 not in want[1:]  # the origin point is skipped
    for block in (512, fr.opt_n_threads(n)):
        assert np.array_equal(fr.fps_as_written(p, m, block), want), block


def test_a_grid_cloud_has_ties_and_they_go_to_the_smallest_index():
    i = np.arange(6, dtype=np.float32)
    whole = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)      # integer coordinates: exact in fp32 and fp64
    out, ties = fr.fps_contract(whole, 40, skip_origin=False, return_ties=True)
    assert ties and np.array_equal(out, brute_force(whole, 40))
    g = i * np.float32(0.02) + np.float32(1)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)          # the 2 cm grid
    out, ties = fr.fps_contract(p, 40, return_ties=True)
    assert ties and out[1] == 215                            # round 1: the far corner, alone
    same = np.zeros((7, 3), dtype=np.float32) + np.float32(2)
    assert list(fr.fps_contract(same, 9)) == [0] * 9
    # the kernel as written resolves the same ties by its tree: one lane is the contract, other block sizes are not
    assert np.array_equal(fr.fps_as_written(p, 40, 1), out)
    assert any(not np.array_equal(fr.fps_as_written(p, 40, b), out) for b in (64, 128, 512))


def test_count_rule_is_pythons_round():
    for r in (0.01, 0.05, 0.1, 0.125, 0.5):
        for n in range(0, 401):
            want = max(5, round(r * n)) if n else 0
            assert fr.count_rule(n, r) == want == annotation.count_rule(n, r)
            assert n == 0 or want == max(5, int(np.rint(np.float64(r) * np.float64(n))))      # the device's spelling
    assert annotation.count_rule(20, 0.125) == 5 and annotation.count_rule(100, 0.125) == 12 and annotation.count_rule(28, 0.125) == 5
    assert round(0.125 * 44) == 6 and round(0.5 * 5) == 2                                    # half to even


def test_symbols_abi_and_tier_bounds():
    L = engine.lib()
    for name in ("lgs_fps_workspace_bytes", "lgs_fps_segments"):
        assert name in engine.EXPORTS and hasattr(L, name)
    assert L.lgs_abi_version() == 18
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    bounds = tuple(int(re.search(r"#define\s+%s\s+(\d+)" % k, txt).group(1))
                   for k in ("LGS_FPS_WAVE_MAX", "LGS_FPS_GROUP4_MAX", "LGS_FPS_GROUP16_MAX"))
    assert bounds == annotation.TIER_BOUNDS
    assert "FPS_FUSED" in tuning.HOST_KNOBS and tuning.HOST_KNOBS["FPS_FUSED"][0] == 1


def test_workspace_bytes_refuses_bad_shapes():
    L = engine.lib()
    assert L.lgs_fps_workspace_bytes(0, 0) > 0 and L.lgs_fps_workspace_bytes(1000, 3) >= 16 * 1000 + 24 * 3
    assert L.lgs_fps_workspace_bytes(1 << 20, 1 << 20) >= (16 + 24) << 20
    for n, s in ((-1, 1), (1, -1), ((1 << 31) - 1, 1), (10, (1 << 20) + 1)):
        assert L.lgs_fps_workspace_bytes(n, s) == 0, (n, s)


def test_segments_refuses_bad_arguments_before_any_device_call():
    L = engine.lib()
    one = ctypes.c_void_p(256)          # never dereferenced: every refusal comes first
    assert L.lgs_fps_segments(None, 10, None, None, 1, None, 5, 0.0, 5, 1, None, None, None, None, None) != 0
    assert b"lgs_fps_segments" in L.lgs_last_error()
    assert L.lgs_fps_segments(None, 10, None, one, 1, None, 5, 0.0, 5, 1, None, one, None, one, None) != 0          # no points
    assert L.lgs_fps_segments(one, 10, None, one, 1, None, 5, 0.0, 5, 1, None, None, None, one, None) != 0          # no output
    assert L.lgs_fps_segments(one, 10, None, one, 1, None, -1, 1.5, 5, 1, None, None, one, one, None) != 0          # ratio
    assert L.lgs_fps_segments(one, 10, None, one, 1, None, -1, float("nan"), 5, 1, None, None, one, one, None) != 0
    assert L.lgs_fps_segments(one, 10, None, one, 1, None, -1, 0.05, -1, 1, None, None, one, one, None) != 0        # min_points
    assert L.lgs_fps_segments(one, 10, None, one, 1, one, -1, 0.05, 5, 1, None, one, None, one, None) != 0          # idx_out, no offsets
    assert L.lgs_fps_segments(one, -1, None, one, 1, None, 5, 0.0, 5, 1, None, one, None, one, None) != 0
    assert L.lgs_fps_segments(one, 10, None, one, (1 << 20) + 1, None, 5, 0.0, 5, 1, None, one, None, one, None) != 0
    with pytest.raises(RuntimeError, match="lgs_fps_segments"):
        engine.check(L.lgs_fps_segments(one, 10, None, one, 1, None, 5, 0.0, 5, 1, None, one, None, None, None))      # no workspace


# ---- the torch path on CPU tensors
def test_torch_lines_equal_the_restatement():
    for n, seed in ((1, 0), (7, 1), (130, 2)):
        p = cloud(n, seed, origin_at=n // 3)
        p[n // 2] = (0.01, 0.02, 0.01)                     # inside the 1e-3 ball
        for m, skip in itertools.product((0, 1, n, n + 3), (True, False)):
            got = annotation.fps_torch(torch.from_numpy(p), m, skip)
            assert got.dtype == torch.int32 and np.array_equal(got.numpy(), fr.fps_contract(p, m, skip)), (n, m, skip)
    g = np.arange(3, dtype=np.float32) * np.float32(0.02) + np.float32(1)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(annotation.fps_torch(torch.from_numpy(grid), 30).numpy(), fr.fps_contract(grid, 30))


def test_batched_form_on_cpu():
    xyz = np.stack([cloud(40, 10 + b) for b in range(3)])
    got = annotation.furthest_point_sample(torch.from_numpy(xyz), 12)
    assert got.shape == (3, 12) and got.dtype == torch.int32
    for b in range(3):
        assert np.array_equal(got[b].numpy(), fr.fps_contract(xyz[b], 12))
    assert annotation.furthest_point_sample(torch.zeros((2, 0, 3)), 4).shape == (2, 4)
    with pytest.raises(ValueError):
        annotation.furthest_point_sample(torch.zeros((2, 5, 3), dtype=torch.float64), 4)


def test_csr_form_on_cpu():
    p = cloud(60, 20, origin_at=11)
    off = [0, 0, 9, 9, 40, 60]
    counts = [3, 4, 0, 35, 5]
    through = torch.from_numpy(np.random.RandomState(3).permutation(60))
    for thr in (None, through):
        want, want_rank = fr.segments_contract(p, off, counts, None if thr is None else thr.numpy())
        idx, out_offsets = annotation.furthest_point_sample_segments(torch.from_numpy(p), off, counts=counts, through=thr)
        assert list(out_offsets.numpy()) == [0, 3, 7, 7, 42, 47]
        for q in range(5):
            got = idx[out_offsets[q]:out_offsets[q + 1]].numpy()
            assert np.array_equal(got[:len(want[q])], want[q]) and not got[len(want[q]):].any()
        # the ratio form: the recipe's counts, per-row ranks
        rule = [fr.count_rule(b - a, 0.125) for a, b in zip(off, off[1:])]
        _, rank_rule = fr.segments_contract(p, off, rule, None if thr is None else thr.numpy())
        rank = annotation.furthest_point_sample_segments(torch.from_numpy(p), torch.tensor(off), ratio=0.125, through=thr)
        assert rank.dtype == torch.int32 and np.array_equal(rank.numpy(), rank_rule)
    with pytest.raises(ValueError):
        annotation.furthest_point_sample_segments(torch.from_numpy(p), off)
    with pytest.raises(ValueError):
        annotation.furthest_point_sample_segments(torch.from_numpy(p), off, counts=counts, ratio=0.1)


def test_limited_annotation_on_cpu():
    p, ids, labels, off = fr.annotation_batch()
    want_labels, want_mask, want_rank = fr.limited_annotation_contract(p, ids, labels, off, 0.1)
    assert want_mask[[3, 50, 88]].all() and 5 <= want_mask[:90][ids[:90] == 0].sum() < (ids[:90] == 0).sum()
    got_labels, got_mask, got_rank = annotation.limited_annotation(torch.from_numpy(p), torch.from_numpy(ids), torch.from_numpy(labels),
                                                                   off, 0.1)
    assert np.array_equal(got_labels.numpy(), want_labels) and np.array_equal(got_mask.numpy(), want_mask)
    assert np.array_equal(got_rank.numpy(), want_rank)
    # the label rule: chosen rows keep their label, the other rows of an instance get the unannotated label, the rest is untouched
    assert np.array_equal(want_labels[ids < 0], labels[ids < 0]) and not want_labels[(ids >= 0) & ~want_mask].any()
    assert np.array_equal(want_labels[want_mask], labels[want_mask]) and not want_mask[ids < 0].any()
    got9 = annotation.limited_annotation(torch.from_numpy(p), torch.from_numpy(ids), torch.from_numpy(labels), off, 0.1,
                                         unannotated_label=255)[0].numpy()
    assert (got9[(ids >= 0) & ~want_mask] == 255).all()
