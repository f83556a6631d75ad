"""lgs_manager_nearest and the point-space evaluation built on it (languagegroundedsemseg_amd/pointcloud.py).

The reference of every comparison is scipy.spatial.cKDTree (or, for tiny cases, a numpy brute force) in float64 on the same float32
inputs, in voxel units: the voxels sit at coords / ts + anchor, the queries are taken there by the same matrix in float64.

The comparison rule.  With d1 <= d2 the reference's two smallest distances of a query:
  distance  the engine's row satisfies dist64(row) <= d1 (1 + 2^-20) for EVERY query;
  row       the engine's row EQUALS the reference's wherever (d2 - d1) / d2 > 1e-5;
  cap       at most 1 % of the queries may be excused from the row comparison, asserted on the reference alone before the engine runs.
Where d2 of the engine is compared with the reference's squared distance the bound is 2e-6 relative (+ 1e-12): the fraction f is
rounded to fp32 once (2^-24 relative) and the five fp32 operations of the sum add 2^-24 each, < 6 * 2^-24 = 3.6e-7 in all, next to
~1e-13 from the different order of the float64 matrix product."""
import functools

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import MinkowskiEngine as ME
from languagegroundedsemseg_amd import engine
from languagegroundedsemseg_amd.metrics import fast_hist
from languagegroundedsemseg_amd.pointcloud import PointCloudEvaluator, nearest_voxel, original_pointcloud_mapping
from languagegroundedsemseg_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.05
TABLES = [1, 0]            # MAP_BLOCK_DIR: the block directory, the hash table


def _similarity(scale=1.0 / VOXEL, yaw=0.3, shift=(1.25, -2.5, 0.75)):
    c, s = np.cos(yaw), np.sin(yaw)
    t = np.eye(4)
    t[:3, :3] = scale * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    t[:3, 3] = shift
    return t


def _tensor(coords):
    c = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).to(DEV)
    return ME.SparseTensor(torch.zeros(c.shape[0], 1, device=DEV), c)


def _reference(sites, site_scene, queries, query_scene):
    """-> (row, d1, d2) per query from one KD-tree per scene (float64); a scene without sites gives row -1, d1 = d2 = inf"""
    row = np.full(len(queries), -1, np.int64)
    d1 = np.full(len(queries), np.inf)
    d2 = np.full(len(queries), np.inf)
    for s in np.unique(query_scene):
        qi, si = np.nonzero(query_scene == s)[0], np.nonzero(site_scene == s)[0]
        if len(si) == 0:
            continue
        d, i = cKDTree(sites[si]).query(queries[qi], k=min(2, len(si)))
        d, i = d.reshape(len(qi), -1), i.reshape(len(qi), -1)
        row[qi], d1[qi] = si[i[:, 0]], d[:, 0]
        if d.shape[1] > 1:
            d2[qi] = d[:, 1]
    return row, d1, d2


def _brute(sites, site_scene, queries, query_scene):
    """the same by numpy brute force, and the smallest row among the exactly equidistant nearest sites"""
    row = np.full(len(queries), -1, np.int64)
    d1 = np.full(len(queries), np.inf)
    d2 = np.full(len(queries), np.inf)
    for i, (q, s) in enumerate(zip(queries, query_scene)):
        si = np.nonzero(site_scene == s)[0]
        if len(si) == 0 or not np.isfinite(q).all():
            continue
        d = np.sqrt(((sites[si] - q[None]) ** 2).sum(1))
        o = np.sort(d)
        d1[i] = o[0]
        d2[i] = o[1] if len(o) > 1 else np.inf
        row[i] = si[d == o[0]].min()
    return row, d1, d2


def _excused(d1, d2):
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(d2), (d2 - d1) / np.where(d2 > 0, d2, 1.0), 1.0)
    return ~(gap > 1e-5)


def _hold(rows, ref, sites, queries):
    """the comparison rule; `ref` = (row, d1, d2) of the reference"""
    ref_row, d1, d2 = ref
    rows = np.asarray(rows)
    has = ref_row >= 0
    assert np.array_equal(rows[~has], ref_row[~has])
    assert (rows[has] >= 0).all() and (rows[has] < len(sites)).all()
    dist = np.sqrt(((sites[rows[has]] - queries[has]) ** 2).sum(1))
    worst = float((dist / np.maximum(d1[has], 1e-300)).max()) if has.any() else 1.0
    print("queries %d  excused %d  worst dist64(row) / d1 - 1 = %.3g" % (len(rows), int(_excused(d1, d2)[has].sum()), worst - 1.0))
    assert (dist <= d1[has] * (1.0 + 2.0 ** -20)).all()
    strict = has & ~_excused(d1, d2)
    assert np.array_equal(rows[strict], ref_row[strict]), "%d rows differ" % int((rows[strict] != ref_row[strict]).sum())


# ---- 1. parity on two synthetic scenes
@functools.lru_cache(None)
def _scenes():
    coords, _, _ = make_batch([0, 1], voxel=VOXEL, n_target=6000)
    coords = coords[np.random.default_rng(5).permutation(len(coords))]          # shuffled: row != sorted position
    assert len(np.unique(coords, axis=0)) == len(coords)
    rng = np.random.default_rng(6)
    v, scene = [], []
    for s in (0, 1):
        c = coords[coords[:, 0] == s][:, 1:].astype(np.float64)
        inside = np.repeat(c, 3, 0) + rng.random((3 * len(c), 3))              # three points inside every occupied cell
        n_far = len(inside) // 20                                               # 5 % far points within +-12 cells of random sites
        far = c[rng.integers(0, len(c), n_far)] + rng.uniform(-12.0, 12.0, (n_far, 3))
        v.append(np.concatenate([inside, far]))
        scene.append(np.full(len(v[-1]), s))
    return coords, np.concatenate(v), np.concatenate(scene)


@functools.lru_cache(None)
def _parity_case(anchor, affine):
    """-> (coords, float32 queries as the engine gets them, scene offsets, 4x4 or None, float64 queries in voxel units, reference)"""
    coords, v, scene = _scenes()
    if affine:
        t = _similarity()
        world = (np.linalg.inv(t) @ np.concatenate([v, np.ones((len(v), 1))], 1).T).T[:, :3]
        q32 = world.astype(np.float32)
        v64 = (t @ np.concatenate([q32.astype(np.float64), np.ones((len(v), 1))], 1).T).T[:, :3]
    else:
        t = None
        q32 = v.astype(np.float32)
        v64 = q32.astype(np.float64)
    sites = coords[:, 1:].astype(np.float64) + anchor
    ref = _reference(sites, coords[:, 0], v64, scene)
    # the cap, on the reference alone
    assert _excused(ref[1], ref[2]).mean() <= 0.01
    off = [0, int((scene == 0).sum()), len(scene)]
    return coords, q32, off, t, v64, sites, ref


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("anchor", [0.0, 0.5])
def test_parity_with_the_kd_tree(anchor, affine, table):
    coords, q32, off, t, v64, sites, ref = _parity_case(anchor, affine)
    with engine.tuning(MAP_BLOCK_DIR=table):
        x = _tensor(coords)
        rows, d2 = nearest_voxel(x, torch.from_numpy(q32).to(DEV), off, None if t is None else torch.from_numpy(t), anchor, return_distance=True)
        rows, d2 = rows.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
        assert x.coordinate_manager._m.check() == 0
    assert np.array_equal(x.C.cpu().numpy(), coords)                             # rows are the inserted order
    _hold(rows, ref, sites, v64)
    assert (coords[rows, 0] == np.repeat([0, 1], np.diff(off))).all()
    own = ((sites[rows] - v64) ** 2).sum(1)
    assert np.allclose(d2, own, rtol=2e-6, atol=1e-12)


# ---- 2. the ring limit changes nothing
@pytest.mark.parametrize("table", TABLES)
def test_every_ring_limit_gives_the_same_answer(table):
    coords, q32, off, t, v64, sites, ref = _parity_case(0.5, False)
    pick = np.concatenate([np.arange(0, off[1], off[1] // 150), np.arange(off[1] - 40, off[1])])   # inside points and far points of scene 0
    q = torch.from_numpy(q32[pick]).to(DEV)
    default = engine.tuning_get("NEAREST_MAX_RING")
    assert default >= 1
    got = []
    for ring in (0, 1, default):
        with engine.tuning(MAP_BLOCK_DIR=table, NEAREST_MAX_RING=ring):
            rows, d2 = nearest_voxel(_tensor(coords), q, None, None, 0.5, return_distance=True)
            got.append((rows.cpu().numpy(), d2.cpu().numpy()))
    for rows, d2 in got[1:]:
        assert np.array_equal(rows, got[0][0])
        assert np.array_equal(d2.view(np.uint32), got[0][1].view(np.uint32))
    _hold(got[0][0], tuple(r[pick] for r in ref), sites, v64[pick])


# ---- 3. exact ties: the smallest row index
def _small(coords, queries, query_scene, anchor=0.0, expect=None, ts_key=False, **kw):
    """one small case against the brute force under the comparison rule, with both tables and ring limits 0 and default"""
    coords = np.asarray(coords, np.int32)
    queries = np.asarray(queries, np.float64)
    q32 = queries.astype(np.float32)
    scenes = np.asarray(query_scene)
    sites = coords[:, 1:].astype(np.float64) + anchor
    base = kw.get("batch_base", 0)
    ref = _brute(sites, coords[:, 0], q32.astype(np.float64), scenes + base)
    assert _excused(ref[1], ref[2])[ref[0] >= 0].mean() <= 0.01 or expect is not None
    b = int(scenes.max()) + 1 if len(scenes) else 1
    off = [int((scenes < s).sum()) for s in range(b + 1)]
    out = []
    for table in TABLES:
        for ring in (0, engine.tuning_get("NEAREST_MAX_RING")):
            with engine.tuning(MAP_BLOCK_DIR=table, NEAREST_MAX_RING=ring):
                rows, d2 = nearest_voxel(_tensor(coords), torch.from_numpy(q32).to(DEV), off, None, anchor, return_distance=True, **kw)
            rows, d2 = rows.cpu().numpy(), d2.cpu().numpy()
            if expect is not None:
                assert np.array_equal(rows, expect), (table, ring, rows, expect)
            else:
                _hold(rows, ref, sites, q32.astype(np.float64))
            out.append((rows, d2))
    for rows, d2 in out[1:]:
        assert np.array_equal(rows, out[0][0]) and np.array_equal(d2.view(np.uint32), out[0][1].view(np.uint32))
    return out[0]


@pytest.mark.parametrize("reverse", [False, True])
def test_exact_ties_go_to_the_smallest_row(reverse):
    g = np.arange(3)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(3).permutation(27)]
    if reverse:
        lattice = lattice[::-1]
    coords = np.concatenate([np.zeros((27, 1), np.int64), lattice], 1)
    q = []
    for a in range(3):                                   # face midpoints: two equidistant sites
        for base in ([0, 1, 1], [1, 1, 1], [1, 0, 2]):
            p = np.array(base, np.float64)
            p[a] = min(p[a], 1.0) + 0.5
            q.append(p)
    for a in range(3):                                   # edge midpoints: four
        for base in ([0, 0, 0], [1, 1, 1], [1, 0, 1]):
            p = np.array(base, np.float64) + 0.5
            p[a] = base[a]
            q.append(p)
    for base in ([0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1]):   # cell midpoints: eight
        q.append(np.array(base, np.float64) + 0.5)
    q = np.array(q)
    d = np.sqrt(((lattice[None].astype(np.float64) - q[:, None]) ** 2).sum(2))    # exact in float64: halves and integers
    ties = d == d.min(1, keepdims=True)
    assert sorted(set(ties.sum(1))) == [2, 4, 8]
    expect = np.array([np.nonzero(t)[0].min() for t in ties])
    _small(coords, q, np.zeros(len(q), np.int64), anchor=0.0, expect=expect)


# ---- 4. borders
def test_borders_of_blocks_and_of_the_sign():
    coords = [[0, 3, 0, 0], [0, 10, 1, 0],               # the nearest site across a 4 x 4 x 4 block border
              [0, -1, 20, 0], [0, 5, 25, 5],             # across the -1 / 0 border
              [0, 3, 40, 3], [0, 4, 40, 4]]              # two blocks meeting at a corner
    q = [[3.6, 0.1, 0.2], [4.4, -0.3, 0.0], [-0.4, 20.2, 0.0], [0.45, 19.8, -0.2], [3.7, 40.4, 3.6], [3.4, 39.9, 3.45]]
    rows, _ = _small(coords, q, [0] * len(q))
    assert list(rows[:4]) == [0, 0, 2, 2]


@pytest.mark.parametrize("shift", [100, -300])
def test_shifted_coordinates(shift):
    rng = np.random.default_rng(11)
    c = np.unique(rng.integers(-6, 7, (400, 3)), axis=0)
    c = c[rng.permutation(len(c))] + shift
    coords = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    q = c[rng.integers(0, len(c), 300)] + rng.uniform(-2.5, 2.5, (300, 3))
    _small(coords, q, np.zeros(300, np.int64), anchor=0.5)


def test_one_isolated_site_far_from_its_query():
    rows, d2 = _small([[0, 7, -2, 3]], [[47.0, -1.8, 3.1], [7.2, -42.0, 3.0]], [0, 0])
    assert list(rows) == [0, 0]
    assert np.allclose(d2, [40.0 ** 2 + 0.2 ** 2 + 0.1 ** 2, 0.2 ** 2 + 40.0 ** 2], rtol=1e-6)


# ---- 5. batches
def test_scenes_never_see_each_other():
    rng = np.random.default_rng(12)
    c = np.unique(rng.integers(0, 9, (150, 3)), axis=0)
    coords = np.concatenate([np.concatenate([np.zeros((len(c), 1), np.int64), c], 1), np.concatenate([np.ones((len(c), 1), np.int64), c + 3], 1)])
    coords = coords[rng.permutation(len(coords))]
    q = rng.uniform(-1.0, 13.0, (400, 3))
    scenes = np.repeat([0, 1], 200)
    rows, _ = _small(coords, q, scenes)
    assert (coords[rows, 0] == scenes).all()


def test_batch_base_selects_the_scene():
    rng = np.random.default_rng(13)
    c = [np.unique(rng.integers(0, 8, (60, 3)), axis=0) for _ in range(3)]
    coords = np.concatenate([np.concatenate([np.full((len(ci), 1), b), ci], 1) for b, ci in enumerate(c)])
    coords = coords[rng.permutation(len(coords))]
    q = rng.uniform(0.0, 8.0, (100, 3))
    rows, _ = _small(coords, q, np.zeros(100, np.int64), batch_base=2)
    assert (coords[rows, 0] == 2).all()
    rows, _ = _small(coords, q, np.repeat([0, 1], 50), batch_base=1)
    assert (coords[rows, 0] == np.repeat([1, 2], 50)).all()


def test_a_scene_without_sites_and_points_that_are_no_numbers():
    coords = [[0, 0, 0, 0], [0, 1, 0, 0]]
    q = np.array([[0.2, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [0.9, 0.1, 0.0], [0.5, 0.5, 0.5]])
    rows, d2 = _small(coords, q, [0, 0, 0, 0, 0, 1], expect=np.array([0, -1, -1, -1, 1, -1]))
    assert np.isposinf(d2[[1, 2, 3, 5]]).all() and np.isfinite(d2[[0, 4]]).all()


@pytest.mark.parametrize("table", TABLES)
def test_no_points_and_no_sites(table):
    with engine.tuning(MAP_BLOCK_DIR=table):
        x = _tensor([[0, 0, 0, 0], [0, 1, 0, 0]])
        rows, d2 = nearest_voxel(x, torch.zeros(0, 3, device=DEV), None, None, 0.5, return_distance=True)
        assert rows.shape == (0,) and rows.dtype == torch.int64 and d2.shape == (0,)
        cm = ME.CoordinateManager(D=3, device=DEV)
        key, _ = cm.insert_and_map(torch.zeros(0, 4, dtype=torch.int32, device=DEV))
        rows, d2 = nearest_voxel((cm, key), torch.rand(5, 3, device=DEV), None, None, 0.5, return_distance=True)
        assert rows.tolist() == [-1] * 5 and torch.isposinf(d2).all()


# ---- 6. a coarser map of the same tensor
@pytest.mark.parametrize("table", TABLES)
def test_a_stride_two_map(table):
    coords, q32, off, _, _, _, _ = _parity_case(0.5, False)
    pick = np.arange(0, len(q32), 7)
    scenes = np.repeat([0, 1], np.diff(off))[pick]
    with engine.tuning(MAP_BLOCK_DIR=table):
        x = _tensor(coords)
        cm = x.coordinate_manager
        key2 = cm.stride(x.coordinate_map_key, 2)
        c2 = cm.get_coordinates(key2).cpu().numpy()
        assert (c2[:, 1:] % 2 == 0).all() and key2.get_tensor_stride() == [2, 2, 2]
        sites = c2[:, 1:].astype(np.float64) / 2.0 + 0.5
        v64 = q32[pick].astype(np.float64) / 2.0
        ref = _reference(sites, c2[:, 0], v64, scenes)
        assert _excused(ref[1], ref[2]).mean() <= 0.01
        o2 = [0, int((scenes == 0).sum()), len(scenes)]
        rows = nearest_voxel((cm, key2), torch.from_numpy(q32[pick]).to(DEV), o2, None, 0.5)
    _hold(rows.cpu().numpy(), ref, sites, v64)


# ---- 7. the two call sites of the reference
def test_original_pointcloud_mapping_is_the_insseg_argmin():
    rng = np.random.default_rng(21)
    c = np.unique(rng.integers(-10, 10, (4500, 3)), axis=0)[:3000]
    c = c[rng.permutation(len(c))]
    coords = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    t = _similarity(scale=1.0 / 0.02, yaw=1.1, shift=(3.0, -7.0, 0.5))
    y = (np.linalg.inv(t) @ np.concatenate([c + 0.5, np.ones((len(c), 1))], 1).T).T[:, :3]        # the reference's lines 155-158
    x32 = (y[rng.integers(0, len(y), 2000)] + rng.normal(0.0, 0.02, (2000, 3))).astype(np.float32)
    d = np.sqrt(((x32.astype(np.float64)[:, None] - y[None]) ** 2).sum(2))                        # D_ij of line 167, in float64
    o = np.sort(d, 1)
    ref = (d.argmin(1), o[:, 0], o[:, 1])
    assert _excused(ref[1], ref[2]).mean() <= 0.01
    sinput = _tensor(coords)
    transformation = torch.from_numpy(np.concatenate([t.reshape(1, 16), np.zeros((1, 4))], 1))   # collate's row: 16 values and more
    query = torch.from_numpy(x32).to(DEV)
    inds, back = original_pointcloud_mapping(sinput, transformation, query)
    assert back is query and inds.dtype == torch.int64
    _hold(inds.cpu().numpy(), ref, y, x32.astype(np.float64))


def test_evaluator_matches_fast_hist_of_kd_tree_labels():
    rng = np.random.default_rng(22)
    n_labels = 7
    c = np.unique(rng.integers(-12, 12, (2500, 3)), axis=0)
    c = c[rng.permutation(len(c))]
    coords = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    scores = rng.standard_normal((len(c), n_labels)).astype(np.float32)
    pred = scores.argmax(1)
    world = (c[rng.integers(0, len(c), 5000)] + rng.uniform(-1.5, 1.5, (5000, 3))) * VOXEL
    q32 = world.astype(np.float32)
    labels = rng.integers(-1, n_labels, 5000)
    d, result = cKDTree(c.astype(np.float64) * VOXEL).query(q32.astype(np.float64), k=2)           # test_pointcloud: pred[:, :3] *= voxel_size
    assert ((d[:, 1] - d[:, 0]) / d[:, 1] > 1e-5).all()                                            # no query the rule would excuse
    want = fast_hist(pred[result[:, 0]], labels, n_labels)
    ev = PointCloudEvaluator(n_labels, ignore_label=-1).to(DEV)
    scale = np.eye(4)
    scale[:3, :3] /= VOXEL
    x = _tensor(coords)
    half = 2500
    for lo, hi in ((0, half), (half, 5000)):                                                       # two updates accumulate
        got = ev.update(torch.from_numpy(scores).to(DEV), x, torch.from_numpy(q32[lo:hi]).to(DEV), torch.from_numpy(labels[lo:hi]).to(DEV),
                        transformation=scale, anchor=0.0)
        assert np.array_equal(got.cpu().numpy(), pred[result[lo:hi, 0]])
    assert ev.confmat.dtype == torch.int64 and np.array_equal(ev.confmat.cpu().numpy(), want)
    assert int(ev.compute()["count"]) == int((labels >= 0).sum())


def test_refusals_of_the_python_layer():
    x = _tensor([[0, 0, 0, 0], [0, 1, 0, 0]])
    pts = torch.rand(4, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="similarity"):
        nearest_voxel(x, pts, transformation=np.diag([20.0, 20.0, 10.0, 1.0]))
    with pytest.raises(RuntimeError, match="HIP tensor|no CPU fallback"):
        nearest_voxel(x, pts.cpu())
    with pytest.raises(RuntimeError):
        original_pointcloud_mapping(x, torch.eye(4), pts.cpu())
