"""The view gain's numpy twin (qn_amd/mapview.py) against the definition - its brute(), a Python loop over mapoccupancy.walk - and against what the construction
of each case of tests/view_cases.py determines.  Pure numpy, no GPU."""
import numpy as np
import pytest
import view_cases as vc
from qn_amd import mapoccupancy as mo, mapview as mv


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("g", vc.NAMES)
def test_gain_equals_brute_and_the_expectations(g):
    for c in vc.group(g):
        cls, grid = vc.inputs(c.name)
        got = vc.twin(c.name)
        want = mv.brute(cls, grid, c.viewpoints, c.offsets, c.params)
        assert _same(got["info"], want["info"]) and _same(got["cover"], want["cover"]) and got["stats"] == want["stats"], c.name
        for r in (got, want):
            vc.holds(c, r["info"], r["cover"], r["stats"]._asdict())


def test_the_starred_rows_by_the_walk_itself():
    """the voxels the issue's knife edges name, straight from mapoccupancy.walk"""
    assert mo.walk((512, 512, 512), (512 + 1024, 512 + 1024, 512)) == [(0, 0, 0), (1, 0, 0), (1, 1, 0)]                # the tie goes to the lowest axis
    assert mo.walk((1024, 512, 512), (512, 512, 512)) == [(1, 0, 0), (0, 0, 0)]                                      # on a face heading down: at once
    assert mo.walk((1024, 512, 512), (2048, 512, 512)) == [(1, 0, 0), (2, 0, 0)]
    assert [v[0] for v in mo.walk((512, 512, 512), (512 + 6 * 1024, 512, 512))] == list(range(7))
    assert mo.walk((512, 512, 512), (512, 512, 512)) == [(0, 0, 0)]


def test_a_random_volume_with_a_shifted_grid():
    """a seeded random three-class 6 x 12 x 14 volume whose voxel (0, 0, 0) is not the world's, voxel 0.3: 300 random offsets, 4 viewpoints"""
    rng = np.random.default_rng(5)
    cls = rng.choice(np.array([0, 1, 2], np.uint8), size=(6, 12, 14), p=(0.5, 0.4, 0.1))
    minc = (-5, 3, -2)
    grid = mo.OccupancyGrid(tuple(m * 0.3 for m in minc), 0.3, 14, 12, 6, minc)
    vps = (rng.uniform([0, 0, 0], [14, 12, 6], size=(4, 3)) + np.array(minc)) * 0.3
    off = rng.integers(-20 * 1024, 20 * 1024, size=(300, 3)).astype(np.int32)
    for p in (mv.ViewParams(), mv.ViewParams(max_through=3, iz_lo=2, iz_hi=4), mv.ViewParams(2, 0, 0, 0, 5)):
        got, want = mv.gain(cls, grid, vps, off, p), mv.brute(cls, grid, vps, off, p)
        assert _same(got["info"], want["info"]) and _same(got["cover"], want["cover"]) and got["stats"] == want["stats"], p
        assert got["stats"].outside == 0 and got["stats"].total_gain == int(got["info"]["gain"].sum()) > 0


def test_sensor_offsets_are_beam_major_and_refuse_beyond_the_limit():
    off = mv.sensor_offsets(0.3, 20.0, 16, 300, -15, 15)
    assert off.dtype == np.int32 and off.shape == (16 * 300, 3)
    assert (off[:300, 2] == off[0, 2]).all() and off[0, 2] < 0 < off[-1, 2] and (np.diff(off[::300, 2]) > 0).all()      # a beam's rows are back to back, elevation rising
    assert off[0].tolist() == [int(np.rint(np.cos(np.deg2rad(-15.0)) * (20.0 / 0.3) * 1024.0)), 0, int(np.rint(np.sin(np.deg2rad(-15.0)) * (20.0 / 0.3) * 1024.0))]
    assert off[75, 0] in (-1, 0, 1) and off[75, 1] > 0                                                                   # a quarter turn: +y
    assert int(np.abs(off).max()) <= int(np.rint(20.0 / 0.3 * 1024.0))
    one = mv.sensor_offsets(1.0, 32768.0, 1, 4, 0, 0)
    assert np.abs(one).max() == mv.MAX_OFFSET
    with pytest.raises(ValueError):
        mv.sensor_offsets(1.0, 32769.0, 1, 4, 0, 0)
    with pytest.raises(ValueError):
        mv.sensor_offsets(0.001, 60.0, 16, 300, -15, 15)


def test_the_arguments_are_checked():
    cls = np.zeros((1, 1, 2), np.uint8); grid = mo.OccupancyGrid((0.0, 0.0, 0.0), 1.0, 2, 1, 1, (0, 0, 0))
    v, o = [[0.5, 0.5, 0.5]], [[1024, 0, 0]]
    for bad in (dict(gain_mask=0), dict(gain_mask=8), dict(stop_mask=8), dict(stop_mask=1), dict(gain_mask=5, stop_mask=4), dict(iz_lo=3, iz_hi=2), dict(max_through=1 << 32)):
        with pytest.raises(ValueError):
            mv.gain(cls, grid, v, o, mv.ViewParams(**bad))
    for off in ([[mv.MAX_OFFSET + 1, 0, 0]], [[0, -mv.MAX_OFFSET - 1, 0]], np.zeros((0, 3), np.int32), [[1, 2]]):
        with pytest.raises(ValueError):
            mv.gain(cls, grid, v, off)
    with pytest.raises(ValueError):
        mv.gain(cls, grid, np.zeros((0, 3)), o)
    assert mv.gain(cls, grid, v, o)["info"]["gain"].tolist() == [2] and mv.ViewParams() == (1, 4, 0, 0, 0x7fffffff)
